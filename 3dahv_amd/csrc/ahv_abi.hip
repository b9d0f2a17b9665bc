// ahv_abi.hip -- the C ABI declared in include/ahv.h: argument validation, error
// strings, launches.  No allocation, no host synchronisation, no exceptions.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/ahv.h"
#include "../../include/ahv_diag.h"
#include "ahv_launch.h"

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(const char* what, hipError_t e)
{
    return fail(AHV_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// CU count of the current device, cached per device id.
int cu_count()
{
    static thread_local int cached_dev = -1, cached_cu = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (dev != cached_dev) {
        int cu = 0;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0)
            return -1;
        cached_dev = dev;
        cached_cu = cu;
    }
    return cached_cu;
}

// A pointer some kernel reads through a vector type without testing the address: refused here, never launched misaligned.
bool misaligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) != 0; }

}  // namespace

extern "C" {

int ahv_abi_version(void) { return (2 << 16) | 3; }

const char* ahv_last_error(void) { return g_err; }

int ahv_device_cu_count(void)
{
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    return cu;
}

// hipMemsetAsync is not used anywhere in the library: see zero_fill_kernel (ahv_ops.hip).
static hipError_t zero_span(void* p, size_t bytes, hipStream_t s)
{
    void* const ptrs[1] = {p};
    const size_t n[1] = {bytes};
    return ahv::launch_zero_fill(ptrs, n, 1, s);
}

// tgt = target features (tgt_is_volume = false) or the target volume (ahv_verify_pair_f32)
static int score_common(const char* who, const float* vol_src, const float* tgt, bool tgt_is_volume, const float* R,
                        int64_t r_batch_stride, int64_t n_offset, const float* W1, const float* W2, const float* b2, int B,
                        int64_t N, float* scores, int64_t* best_key, float* feat_tgt_out, unsigned flags,
                        uint64_t* clock_stamps, void* stream)
{
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "%s: negative size (B=%d, N=%lld)", who, B, (long long)N);
    if (B > 0 && N > 0 && (!vol_src || !tgt || !R || !W1 || !W2 || !b2))
        return fail(AHV_EINVAL, "%s: null input pointer", who);
    if (r_batch_stride != 0 && r_batch_stride < N * 9)
        return fail(AHV_EINVAL, "%s: r_batch_stride %lld must be 0 or >= N*9", who, (long long)r_batch_stride);
    if (n_offset < 0 || n_offset + N > 4294967296ll)
        return fail(AHV_EINVAL, "%s: n_offset + N must fit in 32 bits", who);
    if (flags & ~(AHV_SCORE_RESET_BEST | AHV_SCORE_SPLIT_F16 | AHV_SCORE_NO_TEAMS | AHV_SCORE_SPARE_CUS_MASK))
        return fail(AHV_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (tgt_is_volume && misaligned(tgt, 8))   // tgt_regs_load<true> reads it as float2
        return fail(AHV_EINVAL, "%s: vol_tgt must be 8-byte aligned", who);
    const bool split = (flags & AHV_SCORE_SPLIT_F16) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (best_key && (flags & AHV_SCORE_RESET_BEST) && B > 0) {
        hipError_t e = ahv::launch_fill_keys(best_key, B, s);
        if (e != hipSuccess) return hip_fail("score: key reset", e);
    }
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    if (tgt_is_volume && split) {
        // the split-f16 kernel takes ready-made target features: two launches, through the caller's buffer
        if (B > 0 && !feat_tgt_out)
            return fail(AHV_EINVAL, "%s: AHV_SCORE_SPLIT_F16 needs feat_tgt_out (the target features go through it)", who);
        if (B > 0) {
            hipError_t e = ahv::launch_forward_3d2d(tgt, W1, W2, b2, B, feat_tgt_out, cu, s);
            if (e != hipSuccess) return hip_fail("verify_pair: forward_3d2d launch", e);
        }
        tgt = feat_tgt_out;
        tgt_is_volume = false;
        feat_tgt_out = nullptr;
    }
    if (B == 0) return AHV_OK;
    if (N == 0 && !(tgt_is_volume && feat_tgt_out)) return AHV_OK;  // nothing to score (verify_pair still owes the features)
    ahv::ScoreLaunch a;
    a.vol_src = vol_src; a.tgt = tgt; a.tgt_is_volume = tgt_is_volume; a.R = R;
    a.r_batch_stride = r_batch_stride; a.n_offset = n_offset; a.W1 = W1; a.W2 = W2; a.b2 = b2; a.B = B; a.N = N;
    a.scores = scores; a.best_key = best_key; a.feat_tgt_out = feat_tgt_out; a.num_cu = cu;
    a.spare_cu = (int)((flags & AHV_SCORE_SPARE_CUS_MASK) >> AHV_SCORE_SPARE_CUS_SHIFT);
    a.split_f16 = split; a.no_teams = (flags & AHV_SCORE_NO_TEAMS) != 0; a.clock_stamps = clock_stamps;
    hipError_t e = ahv::launch_score_hypotheses(a, s);
    if (e != hipSuccess) return hip_fail("score: launch", e);
    return AHV_OK;
}

int ahv_score_hypotheses_f32(const float* vol_src, const float* feat_tgt, const float* R,
                             int64_t r_batch_stride, int64_t n_offset, const float* W1, const float* W2,
                             const float* b2, int B, int64_t N, float* scores, int64_t* best_key,
                             unsigned flags, void* stream)
{
    return score_common("score", vol_src, feat_tgt, false, R, r_batch_stride, n_offset, W1, W2, b2, B, N, scores, best_key,
                        nullptr, flags, nullptr, stream);
}

int ahv_score_hypotheses_clocked_f32(const float* vol_src, const float* feat_tgt, const float* R,
                                     int64_t r_batch_stride, int64_t n_offset, const float* W1, const float* W2,
                                     const float* b2, int B, int64_t N, float* scores, int64_t* best_key,
                                     unsigned flags, uint64_t* clock_stamps, void* stream)
{
    if (!clock_stamps) return fail(AHV_EINVAL, "score_clocked: null clock_stamps");
    return score_common("score_clocked", vol_src, feat_tgt, false, R, r_batch_stride, n_offset, W1, W2, b2, B, N, scores,
                        best_key, nullptr, flags, clock_stamps, stream);
}

int ahv_diag_score_plan(int B, int64_t N, unsigned flags, int* gx, int* gy, int64_t* n_main)
{
    if (B < 1 || N < 0) return fail(AHV_EINVAL, "score_plan: bad shape (B=%d, N=%lld)", B, (long long)N);
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    const bool teams = !(flags & AHV_SCORE_SPLIT_F16) && !(flags & AHV_SCORE_NO_TEAMS);
    const ahv::ScorePlan p = ahv::plan_score_launch(B, N, cu, (int)((flags & AHV_SCORE_SPARE_CUS_MASK) >> AHV_SCORE_SPARE_CUS_SHIFT), teams);
    if (gx) *gx = p.gx;
    if (gy) *gy = p.gy;
    if (n_main) *n_main = p.n_main;
    return AHV_OK;
}

int ahv_verify_pair_f32(const float* vol_src, const float* vol_tgt, const float* R, int64_t r_batch_stride,
                        int64_t n_offset, const float* W1, const float* W2, const float* b2, int B, int64_t N,
                        float* scores, int64_t* best_key, float* feat_tgt_out, unsigned flags, uint64_t* clock_stamps,
                        void* stream)
{
    return score_common("verify_pair", vol_src, vol_tgt, true, R, r_batch_stride, n_offset, W1, W2, b2, B, N, scores,
                        best_key, feat_tgt_out, flags, clock_stamps, stream);
}

int ahv_unpack_best(const int64_t* best_key, int B, float* best_score, int64_t* best_idx, void* stream)
{
    if (!best_key) return fail(AHV_EINVAL, "unpack: null best_key");
    if (B < 0) return fail(AHV_EINVAL, "unpack: negative B");
    if (B == 0) return AHV_OK;
    hipError_t e = ahv::launch_unpack_best(best_key, B, best_score, best_idx, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("unpack: launch", e);
    return AHV_OK;
}

int ahv_rotate_volume_f32(const float* vol, int64_t vol_batch_stride, const float* R, int64_t N, int C, int D,
                          int H, int W, float* out, void* stream)
{
    if (N < 0 || C < 1 || D < 1 || H < 1 || W < 1)
        return fail(AHV_EINVAL, "rotate_volume: bad shape N=%lld C=%d D=%d H=%d W=%d", (long long)N, C, D, H, W);
    if (vol_batch_stride != 0 && vol_batch_stride < (int64_t)C * D * H * W)
        return fail(AHV_EINVAL, "rotate_volume: vol_batch_stride = %lld: the batch stride must be 0 or >= C*D*H*W", (long long)vol_batch_stride);
    if (N == 0) return AHV_OK; /* empty batch: nothing to read or write, pointers may be null */
    if (!vol || !R || !out) return fail(AHV_EINVAL, "rotate_volume: null pointer");
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    hipError_t e = ahv::launch_rotate_volume(vol, vol_batch_stride, R, N, C, D, H, W, out, cu,
                                             static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("rotate_volume: launch", e);
    return AHV_OK;
}

int ahv_rotate_volume_backward_f32(const float* grad_out, int64_t vol_batch_stride, const float* R, int64_t N, int C,
                                   int D, int H, int W, float* grad_vol, void* stream)
{
    if (N < 0 || C < 1 || D < 1 || H < 1 || W < 1)
        return fail(AHV_EINVAL, "rotate_volume_backward: bad shape N=%lld C=%d D=%d H=%d W=%d", (long long)N, C, D, H, W);
    const int64_t vol_elems = (int64_t)C * D * H * W;
    if (vol_batch_stride != 0 && vol_batch_stride < vol_elems)
        return fail(AHV_EINVAL, "rotate_volume_backward: vol_batch_stride = %lld: the batch stride must be 0 or >= C*D*H*W", (long long)vol_batch_stride);
    if (!grad_vol) return fail(AHV_EINVAL, "rotate_volume_backward: null grad_vol");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n_vol = vol_batch_stride == 0 ? 1 : N;
    if (n_vol > 0) {
        // packed volumes are one span; strided ones are zeroed volume by volume: the caller's bytes between them stay
        const bool packed = vol_batch_stride == 0 || vol_batch_stride == vol_elems;
        hipError_t e = packed ? zero_span(grad_vol, sizeof(float) * (size_t)(n_vol * vol_elems), s)
                              : ahv::launch_zero_fill_strided(grad_vol, vol_elems, vol_batch_stride, n_vol, s);
        if (e != hipSuccess) return hip_fail("rotate_volume_backward: zero fill", e);
    }
    if (N == 0) return AHV_OK;
    if (!grad_out || !R) return fail(AHV_EINVAL, "rotate_volume_backward: null pointer");
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    hipError_t e = ahv::launch_rotate_volume_backward(grad_out, vol_batch_stride, R, N, C, D, H, W, grad_vol, cu, s);
    if (e != hipSuccess) return hip_fail("rotate_volume_backward: launch", e);
    return AHV_OK;
}

int ahv_rotate_volume_rotation_grad_f32(const float* grad_out, const float* vol, int64_t vol_batch_stride, const float* R,
                                        int64_t N, int C, int D, int H, int W, float* grad_R, void* stream)
{
    if (N < 0 || C < 1 || D < 1 || H < 1 || W < 1)
        return fail(AHV_EINVAL, "rotate_volume_rotation_grad: bad shape N=%lld C=%d D=%d H=%d W=%d", (long long)N, C, D, H, W);
    if (vol_batch_stride != 0 && vol_batch_stride < (int64_t)C * D * H * W)
        return fail(AHV_EINVAL, "rotate_volume_rotation_grad: vol_batch_stride = %lld: the batch stride must be 0 or >= C*D*H*W", (long long)vol_batch_stride);
    if (N == 0) return AHV_OK; /* nothing to read or write, pointers may be null */
    if (!grad_out || !vol || !R || !grad_R) return fail(AHV_EINVAL, "rotate_volume_rotation_grad: null pointer");
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    hipError_t e = ahv::launch_rotate_volume_rotation_grad(grad_out, vol, vol_batch_stride, R, N, C, D, H, W, grad_R, cu,
                                                           static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("rotate_volume_rotation_grad: launch", e);
    return AHV_OK;
}

int ahv_forward_3d2d_f32(const float* vol, const float* W1, const float* W2, const float* b2, int64_t M,
                         float* out, void* stream)
{
    if (M < 0) return fail(AHV_EINVAL, "forward_3d2d: negative M");
    if (M == 0) return AHV_OK;
    if (!vol || !W1 || !W2 || !b2 || !out) return fail(AHV_EINVAL, "forward_3d2d: null pointer");
    if (misaligned(vol, 8)) return fail(AHV_EINVAL, "forward_3d2d: vol must be 8-byte aligned");   // staged as float2
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    hipError_t e = ahv::launch_forward_3d2d(vol, W1, W2, b2, M, out, cu, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("forward_3d2d: launch", e);
    return AHV_OK;
}

int ahv_score_features_f32(const float* f_src, const float* f_tgt, int B, int64_t N, float* scores, void* stream)
{
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "score_features: negative size");
    if (B == 0 || N == 0) return AHV_OK;
    if (!f_src || !f_tgt || !scores) return fail(AHV_EINVAL, "score_features: null pointer");
    if (misaligned(f_src, 16)) return fail(AHV_EINVAL, "score_features: f_src must be 16-byte aligned");   // read as float4
    if (misaligned(f_tgt, 16)) return fail(AHV_EINVAL, "score_features: f_tgt must be 16-byte aligned");
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    hipError_t e = ahv::launch_score_features(f_src, f_tgt, B, N, scores, cu, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("score_features: launch", e);
    return AHV_OK;
}

int ahv_compose_rotations_f32(const int64_t* best_key, const float* R, int64_t r_batch_stride, int64_t n_offset,
                                 int64_t N, const float* D, int64_t N2, int B, float* out, void* stream)
{
    if (B < 0 || N < 0 || N2 < 0) return fail(AHV_EINVAL, "compose_rotations: negative size");
    if (B == 0 || N2 == 0) return AHV_OK;
    if (!best_key || !R || !D || !out) return fail(AHV_EINVAL, "compose_rotations: null pointer");
    if (N == 0) return fail(AHV_EINVAL, "compose_rotations: empty rotation set");
    if (r_batch_stride != 0 && r_batch_stride < N * 9) return fail(AHV_EINVAL, "compose_rotations: r_batch_stride %lld must be 0 or >= N*9", (long long)r_batch_stride);
    hipError_t e = ahv::launch_compose_rotations_topk(best_key, 1, R, r_batch_stride, n_offset, N, D, N2, B, out,
                                                      static_cast<hipStream_t>(stream));  // one seed: the list at K = 1
    if (e != hipSuccess) return hip_fail("compose_rotations: launch", e);
    return AHV_OK;
}

int ahv_coarse_to_fine_f32(const float* vol_src, const float* vol_tgt, const float* R, int64_t r_batch_stride, int64_t N,
                           const float* D, int64_t N2, const float* W1, const float* W2, const float* b2, int B,
                           float* scores_coarse, float* scores_fine, int64_t* keys, uint32_t* sync, float* feat_tgt_out,
                           float* R_pred, float* fine_score, int64_t* fine_idx, float* coarse_score, int64_t* coarse_idx,
                           unsigned flags, void* stream)
{
    if (B < 0 || N < 0 || N2 < 0) return fail(AHV_EINVAL, "coarse_to_fine: negative size (B=%d, N=%lld, N2=%lld)", B, (long long)N, (long long)N2);
    if (B == 0) return AHV_OK;
    if (N == 0 || N2 == 0) return fail(AHV_EINVAL, "coarse_to_fine: empty hypothesis set (N=%lld, N2=%lld)", (long long)N, (long long)N2);
    if (!vol_src || !vol_tgt || !R || !D || !W1 || !W2 || !b2) return fail(AHV_EINVAL, "coarse_to_fine: null input pointer");
    if (!keys || !sync) return fail(AHV_EINVAL, "coarse_to_fine: keys and sync are required (2 B keys, 2 B + 1 counters)");
    if (r_batch_stride != 0 && r_batch_stride < N * 9)
        return fail(AHV_EINVAL, "coarse_to_fine: r_batch_stride %lld must be 0 or >= N*9", (long long)r_batch_stride);
    if (N > 4294967296ll || N2 > 4294967296ll) return fail(AHV_EINVAL, "coarse_to_fine: indices must fit in 32 bits");
    if (flags & ~(AHV_SCORE_NO_TEAMS | AHV_SCORE_SPARE_CUS_MASK)) return fail(AHV_EINVAL, "coarse_to_fine: unknown flags 0x%x", flags);
    if (misaligned(vol_tgt, 8)) return fail(AHV_EINVAL, "coarse_to_fine: vol_tgt must be 8-byte aligned");
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    ahv::CoarseToFineLaunch a;
    ahv::ScoreLaunch& c = a.coarse;
    c.vol_src = vol_src; c.tgt = vol_tgt; c.tgt_is_volume = true; c.R = R; c.r_batch_stride = r_batch_stride; c.n_offset = 0;
    c.W1 = W1; c.W2 = W2; c.b2 = b2; c.B = B; c.N = N; c.scores = scores_coarse; c.best_key = keys;
    c.feat_tgt_out = feat_tgt_out; c.num_cu = cu;
    c.spare_cu = (int)((flags & AHV_SCORE_SPARE_CUS_MASK) >> AHV_SCORE_SPARE_CUS_SHIFT);
    c.split_f16 = false; c.no_teams = (flags & AHV_SCORE_NO_TEAMS) != 0; c.clock_stamps = nullptr;
    a.D = D; a.N2 = N2; a.scores2 = scores_fine; a.best_key2 = keys + B; a.sync = sync; a.R_pred = R_pred;
    a.fine_score = fine_score; a.coarse_score = coarse_score; a.fine_idx = fine_idx; a.coarse_idx = coarse_idx;
    hipError_t e = ahv::launch_coarse_to_fine(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("coarse_to_fine: launch", e);
    return AHV_OK;
}

int ahv_reset_best(int64_t* best_key, int B, void* stream)
{
    if (B < 0) return fail(AHV_EINVAL, "reset_best: negative B");
    if (B == 0) return AHV_OK;
    if (!best_key) return fail(AHV_EINVAL, "reset_best: null best_key");
    hipError_t e = ahv::launch_fill_keys(best_key, B, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("reset_best: launch", e);
    return AHV_OK;
}

int ahv_select_rotation_f32(int64_t* best_key, const float* R, int64_t r_batch_stride, int64_t n_offset, int64_t N,
                            int B, float* R_out, float* best_score, int64_t* best_idx, unsigned flags, void* stream)
{
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "select_rotation: negative size");
    if (flags & ~AHV_SELECT_RESET_KEY) return fail(AHV_EINVAL, "select_rotation: unknown flags 0x%x", flags);
    if (B == 0) return AHV_OK;
    if (!best_key) return fail(AHV_EINVAL, "select_rotation: null best_key");
    if (R_out && (!R || N == 0)) return fail(AHV_EINVAL, "select_rotation: R_out needs a rotation set");
    if (r_batch_stride != 0 && r_batch_stride < N * 9) return fail(AHV_EINVAL, "select_rotation: r_batch_stride %lld must be 0 or >= N*9", (long long)r_batch_stride);
    hipError_t e = ahv::launch_select_topk(best_key, 1, R, r_batch_stride, n_offset, N, B, R_out, best_score, best_idx,
                                           (flags & AHV_SELECT_RESET_KEY) != 0, static_cast<hipStream_t>(stream));  // B lists of one
    if (e != hipSuccess) return hip_fail("select_rotation: launch", e);
    return AHV_OK;
}

size_t ahv_transformer_workspace_bytes(int B) { return sizeof(float) * ahv::transformer_workspace_floats(B); }

int ahv_transformer_blocks_f32(const ahv_block_weights* blocks, int depth, float* x_src, float* x_tgt, int B,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    if (depth < 0 || B < 0) return fail(AHV_EINVAL, "transformer_blocks: negative size");
    if (depth == 0 || B == 0) return AHV_OK;
    if (!blocks || !x_src || !x_tgt || !workspace) return fail(AHV_EINVAL, "transformer_blocks: null pointer");
    if (workspace_bytes < ahv_transformer_workspace_bytes(B))
        return fail(AHV_EINVAL, "transformer_blocks: workspace of %zu bytes, need %zu", workspace_bytes,
                    ahv_transformer_workspace_bytes(B));
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(x_src) & 15) ||
        (reinterpret_cast<uintptr_t>(x_tgt) & 15))
        return fail(AHV_EINVAL, "transformer_blocks: buffers must be 16-byte aligned");
    for (int i = 0; i < 4 * depth; ++i) {
        const ahv_block_weights& w = blocks[i];
        if (!w.w_qkv || !w.w_out || !w.b_out || !w.ln1_g || !w.ln1_b || !w.w_ff1 || !w.b_ff1 || !w.w_ff2 || !w.b_ff2 ||
            !w.ln2_g || !w.ln2_b)
            return fail(AHV_EINVAL, "transformer_blocks: null weight pointer in block %d", i);
    }
    const char* what = "";
    const int rc = ahv::transformer_blocks(blocks, depth, x_src, x_tgt, B, static_cast<float*>(workspace),
                                           static_cast<hipStream_t>(stream), &what);
    if (rc != 0) return fail(AHV_ELAUNCH, "transformer_blocks: %s: %s", what, hipGetErrorString((hipError_t)rc));
    return AHV_OK;
}

size_t ahv_forward_2d3d_workspace_bytes(int B) { return sizeof(float) * ahv::forward_2d3d_workspace_floats(B); }

int ahv_forward_2d3d_f32(const ahv_aligner_weights* w, const float* layer4_src, const float* layer4_tgt, int B,
                         void* workspace, size_t workspace_bytes, float* vol_src, float* vol_tgt, void* stream)
{
    if (B < 0) return fail(AHV_EINVAL, "forward_2d3d: negative B");
    if (B == 0) return AHV_OK;
    if (!w || !layer4_src || !layer4_tgt || !workspace || !vol_src || !vol_tgt)
        return fail(AHV_EINVAL, "forward_2d3d: null pointer");
    if (!w->w_emb || !w->w_conv1 || !w->w_conv2 || !w->posemb || !w->gn_g || !w->gn_b || !w->w_in[0] || !w->w_in[1] ||
        !w->b_in[0] || !w->b_in[1] || !w->w_out[0] || !w->w_out[1] || !w->b_out[0] || !w->b_out[1] || !w->w3d_1 ||
        !w->w3d_2 || (w->depth > 0 && !w->blocks))
        return fail(AHV_EINVAL, "forward_2d3d: null weight pointer");
    if (w->depth < 0) return fail(AHV_EINVAL, "forward_2d3d: negative depth");
    if (workspace_bytes < ahv_forward_2d3d_workspace_bytes(B))
        return fail(AHV_EINVAL, "forward_2d3d: workspace of %zu bytes, need %zu", workspace_bytes,
                    ahv_forward_2d3d_workspace_bytes(B));
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(AHV_EINVAL, "forward_2d3d: workspace must be 16-byte aligned");
    const char* what = "";
    const int rc = ahv::forward_2d3d(w, layer4_src, layer4_tgt, B, static_cast<float*>(workspace), vol_src, vol_tgt,
                                     static_cast<hipStream_t>(stream), &what);
    if (rc != 0) return fail(AHV_ELAUNCH, "forward_2d3d: %s: %s", what, hipGetErrorString((hipError_t)rc));
    return AHV_OK;
}

size_t ahv_score_hypotheses_backward_workspace_bytes(int B, int64_t N)
{
    if (B <= 0 || N <= 0) return 0;
    return sizeof(float) * ahv::BackwardWs(B, N, cu_count()).floats();   // the layout: ahv_launch.h
}

static int score_backward_common(const float* vol_src, const float* feat_tgt, const float* R,
                                 int64_t r_batch_stride, const float* W1, const float* W2, const float* b2,
                                 int B, int64_t N, const float* grad_scores, void* workspace,
                                 size_t workspace_bytes, float* grad_vol_src, float* grad_feat_tgt,
                                 float* grad_W1, float* grad_W2, float* grad_b2, void* stream, bool saved_u);

int ahv_score_hypotheses_backward_f32(const float* vol_src, const float* feat_tgt, const float* R,
                                      int64_t r_batch_stride, const float* W1, const float* W2, const float* b2,
                                      int B, int64_t N, const float* grad_scores, void* workspace,
                                      size_t workspace_bytes, float* grad_vol_src, float* grad_feat_tgt,
                                      float* grad_W1, float* grad_W2, float* grad_b2, void* stream)
{
    return score_backward_common(vol_src, feat_tgt, R, r_batch_stride, W1, W2, b2, B, N, grad_scores, workspace, workspace_bytes,
                                 grad_vol_src, grad_feat_tgt, grad_W1, grad_W2, grad_b2, stream, false);
}

int ahv_score_hypotheses_backward_saved_f32(const float* vol_src, const float* feat_tgt, const float* R,
                                            int64_t r_batch_stride, const float* W1, const float* W2, const float* b2,
                                            int B, int64_t N, const float* grad_scores, void* workspace,
                                            size_t workspace_bytes, float* grad_vol_src, float* grad_feat_tgt,
                                            float* grad_W1, float* grad_W2, float* grad_b2, void* stream)
{
    return score_backward_common(vol_src, feat_tgt, R, r_batch_stride, W1, W2, b2, B, N, grad_scores, workspace, workspace_bytes,
                                 grad_vol_src, grad_feat_tgt, grad_W1, grad_W2, grad_b2, stream, true);
}

int ahv_score_hypotheses_train_f32(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                   const float* W1, const float* W2, const float* b2, int B, int64_t N, float* scores,
                                   void* workspace, size_t workspace_bytes, void* stream)
{
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "score_train: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "score_train: B > 65535");
    if (B == 0 || N == 0) return AHV_OK;
    if (!vol_src || !feat_tgt || !R || !W1 || !W2 || !b2 || !scores || !workspace) return fail(AHV_EINVAL, "score_train: null pointer");
    if (r_batch_stride != 0 && r_batch_stride != N * 9) return fail(AHV_EINVAL, "score_train: r_batch_stride must be 0 or N*9");
    if (workspace_bytes < ahv_score_hypotheses_backward_workspace_bytes(B, N))
        return fail(AHV_EINVAL, "score_train: workspace of %zu bytes, need %zu (ahv_score_hypotheses_backward_workspace_bytes)",
                    workspace_bytes, ahv_score_hypotheses_backward_workspace_bytes(B, N));
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(AHV_EINVAL, "score_train: workspace must be 16-byte aligned");
    const int cu = cu_count();
    if (cu <= 0) return fail(AHV_EDEVICE, "score_train: no usable HIP device");
    ahv::ScoreLaunch a{};
    a.vol_src = vol_src; a.tgt = feat_tgt; a.tgt_is_volume = false; a.R = R; a.r_batch_stride = r_batch_stride; a.n_offset = 0;
    a.W1 = W1; a.W2 = W2; a.b2 = b2; a.B = B; a.N = N; a.scores = scores; a.best_key = nullptr; a.feat_tgt_out = nullptr;
    a.num_cu = cu; a.spare_cu = 0; a.split_f16 = false; a.no_teams = true; a.clock_stamps = nullptr;
    hipError_t e = ahv::launch_score_hypotheses_train(a, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("score_train: launch", e);
    return AHV_OK;
}

static int score_backward_common(const float* vol_src, const float* feat_tgt, const float* R,
                                 int64_t r_batch_stride, const float* W1, const float* W2, const float* b2,
                                 int B, int64_t N, const float* grad_scores, void* workspace,
                                 size_t workspace_bytes, float* grad_vol_src, float* grad_feat_tgt,
                                 float* grad_W1, float* grad_W2, float* grad_b2, void* stream, bool saved_u)
{
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "score_backward: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "score_backward: B > 65535");
    if (!grad_W1 || !grad_W2 || !grad_b2) return fail(AHV_EINVAL, "score_backward: null weight-gradient pointer");
    if (B > 0 && (!grad_vol_src || !grad_feat_tgt)) return fail(AHV_EINVAL, "score_backward: null gradient pointer");
    if (B > 0 && N > 0) {
        if (!vol_src || !feat_tgt || !R || !W1 || !W2 || !b2 || !grad_scores || !workspace)
            return fail(AHV_EINVAL, "score_backward: null pointer");
        if (r_batch_stride != 0 && r_batch_stride != N * 9)
            return fail(AHV_EINVAL, "score_backward: r_batch_stride must be 0 or N*9");
        if (workspace_bytes < ahv_score_hypotheses_backward_workspace_bytes(B, N))
            return fail(AHV_EINVAL, "score_backward: workspace of %zu bytes, need %zu", workspace_bytes,
                        ahv_score_hypotheses_backward_workspace_bytes(B, N));
        if (reinterpret_cast<uintptr_t>(workspace) & 15)
            return fail(AHV_EINVAL, "score_backward: workspace must be 16-byte aligned");
    }
    const int cu = cu_count();
    if (cu <= 0) return fail(AHV_EDEVICE, "score_backward: no usable HIP device");
    hipError_t e = ahv::launch_score_backward(vol_src, feat_tgt, R, r_batch_stride, W1, W2, b2, B, N, grad_scores,
                                              static_cast<float*>(workspace),
                                              static_cast<float*>(workspace) + ahv::BackwardWs(B, N, cu).partials_offset(),
                                              grad_vol_src, grad_feat_tgt, grad_W1, grad_W2, grad_b2, cu,
                                              static_cast<hipStream_t>(stream), saved_u);
    if (e != hipSuccess) return hip_fail("score_backward: launch", e);
    return AHV_OK;
}

int ahv_random_rotations_f32(uint64_t seed, uint64_t offset, int64_t N, float* out, void* stream)
{
    if (N < 0) return fail(AHV_EINVAL, "random_rotations: negative N");
    if (N == 0) return AHV_OK;
    if (!out) return fail(AHV_EINVAL, "random_rotations: null pointer");
    hipError_t e = ahv::launch_random_rotations(seed, offset, N, out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("random_rotations: launch", e);
    return AHV_OK;
}

int ahv_so3_grid_f32(int64_t n_total, int64_t offset, int64_t N, float* out, void* stream)
{
    if (N < 0 || offset < 0 || n_total <= 0 || offset + N > n_total)
        return fail(AHV_EINVAL, "so3_grid: need 0 <= offset, 0 <= N, offset + N <= n_total");
    if (N == 0) return AHV_OK;
    if (!out) return fail(AHV_EINVAL, "so3_grid: null pointer");
    hipError_t e = ahv::launch_so3_grid(n_total, offset, N, out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("so3_grid: launch", e);
    return AHV_OK;
}

int ahv_argmax_f32(const float* scores, int B, int64_t N, int64_t n_offset, int64_t* best_key, unsigned flags,
                   void* stream)
{
    if (!scores || !best_key) return fail(AHV_EINVAL, "argmax: null pointer");
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "argmax: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "argmax: B > 65535");
    if (n_offset < 0 || n_offset + N > 4294967296ll) return fail(AHV_EINVAL, "argmax: n_offset + N must fit in 32 bits");
    if (flags & ~AHV_SCORE_RESET_BEST) return fail(AHV_EINVAL, "argmax: unknown flags 0x%x", flags);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((flags & AHV_SCORE_RESET_BEST) && B > 0) {
        hipError_t e = ahv::launch_fill_keys(best_key, B, s);
        if (e != hipSuccess) return hip_fail("argmax: key reset", e);
    }
    if (B == 0 || N == 0) return AHV_OK;
    const int cu = cu_count();
    if (cu < 0) return fail(AHV_EDEVICE, "no usable HIP device");
    hipError_t e = ahv::launch_argmax(scores, B, N, n_offset, best_key, cu, s);
    if (e != hipSuccess) return hip_fail("argmax: launch", e);
    return AHV_OK;
}

// ---- K best hypotheses ---------------------------------------------------------------------------------
static bool bad_k(int K) { return K < 1 || K > AHV_TOPK_MAX_K; }

size_t ahv_topk_workspace_bytes(int B, int64_t N, int K)
{
    if (B <= 0 || N <= 0 || bad_k(K)) return 0;
    const int parts = ahv::topk_parts(N);
    return parts <= 1 ? 0 : sizeof(int64_t) * (size_t)parts * (size_t)B * (size_t)K;
}

int ahv_topk_f32(const float* scores, int B, int64_t N, int64_t n_offset, int K, int64_t* keys, void* workspace,
                 size_t workspace_bytes, unsigned flags, void* stream)
{
    if (bad_k(K)) return fail(AHV_EINVAL, "topk: K = %d outside 1..%d", K, AHV_TOPK_MAX_K);
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "topk: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "topk: B > 65535");
    if (n_offset < 0 || n_offset + N > 4294967296ll) return fail(AHV_EINVAL, "topk: n_offset + N must fit in 32 bits");
    if (flags & ~AHV_TOPK_RESET_LIST) return fail(AHV_EINVAL, "topk: unknown flags 0x%x", flags);
    if (B == 0) return AHV_OK;
    if (!keys || (N > 0 && !scores)) return fail(AHV_EINVAL, "topk: null pointer");
    const size_t need = ahv_topk_workspace_bytes(B, N, K);
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)))
        return fail(AHV_EINVAL, "topk: needs an 8-byte aligned workspace of %zu bytes (ahv_topk_workspace_bytes), got %zu", need,
                    workspace_bytes);
    const bool reset = (flags & AHV_TOPK_RESET_LIST) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {
        if (!reset) return AHV_OK;
        hipError_t e = ahv::launch_fill_keys(keys, B * K, s);
        if (e != hipSuccess) return hip_fail("topk: list reset", e);
        return AHV_OK;
    }
    hipError_t e = ahv::launch_topk(scores, B, N, n_offset, K, keys, static_cast<int64_t*>(workspace), !reset, s);
    if (e != hipSuccess) return hip_fail("topk: launch", e);
    return AHV_OK;
}

int ahv_topk_merge_keys(const int64_t* lists, int P, int B, int K, int64_t* keys, unsigned flags, void* stream)
{
    if (bad_k(K)) return fail(AHV_EINVAL, "topk_merge_keys: K = %d outside 1..%d", K, AHV_TOPK_MAX_K);
    if (B < 0 || P < 0) return fail(AHV_EINVAL, "topk_merge_keys: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "topk_merge_keys: B > 65535");
    if (flags & ~AHV_TOPK_RESET_LIST) return fail(AHV_EINVAL, "topk_merge_keys: unknown flags 0x%x", flags);
    if (B == 0) return AHV_OK;
    if (!keys || (P > 0 && !lists)) return fail(AHV_EINVAL, "topk_merge_keys: null pointer");
    const bool reset = (flags & AHV_TOPK_RESET_LIST) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P == 0) {
        if (!reset) return AHV_OK;
        hipError_t e = ahv::launch_fill_keys(keys, B * K, s);
        if (e != hipSuccess) return hip_fail("topk_merge_keys: list reset", e);
        return AHV_OK;
    }
    hipError_t e = ahv::launch_topk_merge(lists, P, B, K, keys, !reset, s);
    if (e != hipSuccess) return hip_fail("topk_merge_keys: launch", e);
    return AHV_OK;
}

int ahv_select_topk_f32(int64_t* keys, int K, const float* R, int64_t r_batch_stride, int64_t n_offset, int64_t N, int B,
                        float* R_out, float* scores_out, int64_t* idx_out, unsigned flags, void* stream)
{
    if (bad_k(K)) return fail(AHV_EINVAL, "select_topk: K = %d outside 1..%d", K, AHV_TOPK_MAX_K);
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "select_topk: negative size");
    if (flags & ~AHV_SELECT_RESET_KEY) return fail(AHV_EINVAL, "select_topk: unknown flags 0x%x", flags);
    if (B == 0) return AHV_OK;
    if (!keys) return fail(AHV_EINVAL, "select_topk: null keys");
    if (R_out && (!R || N == 0)) return fail(AHV_EINVAL, "select_topk: R_out needs a rotation set");
    if (r_batch_stride != 0 && r_batch_stride < N * 9) return fail(AHV_EINVAL, "select_topk: r_batch_stride %lld must be 0 or >= N*9", (long long)r_batch_stride);
    hipError_t e = ahv::launch_select_topk(keys, K, R, r_batch_stride, n_offset, N, B, R_out, scores_out, idx_out,
                                           (flags & AHV_SELECT_RESET_KEY) != 0, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("select_topk: launch", e);
    return AHV_OK;
}

int ahv_compose_rotations_topk_f32(const int64_t* keys, int K, const float* R, int64_t r_batch_stride, int64_t n_offset,
                                   int64_t N, const float* D, int64_t N2, int B, float* out, void* stream)
{
    if (bad_k(K)) return fail(AHV_EINVAL, "compose_rotations_topk: K = %d outside 1..%d", K, AHV_TOPK_MAX_K);
    if (B < 0 || N < 0 || N2 < 0) return fail(AHV_EINVAL, "compose_rotations_topk: negative size");
    if (B == 0 || N2 == 0) return AHV_OK;
    if (!keys || !R || !D || !out) return fail(AHV_EINVAL, "compose_rotations_topk: null pointer");
    if (N == 0) return fail(AHV_EINVAL, "compose_rotations_topk: empty rotation set");
    if (r_batch_stride != 0 && r_batch_stride < N * 9) return fail(AHV_EINVAL, "compose_rotations_topk: r_batch_stride %lld must be 0 or >= N*9", (long long)r_batch_stride);
    hipError_t e = ahv::launch_compose_rotations_topk(keys, K, R, r_batch_stride, n_offset, N, D, N2, B, out,
                                                      static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("compose_rotations_topk: launch", e);
    return AHV_OK;
}

// ---- distinct pose modes ---------------------------------------------------------------------------------
size_t ahv_topk_modes_workspace_bytes(int B, int64_t N, int K)
{
    if (B <= 0 || N <= 0 || bad_k(K)) return 0;
    return sizeof(int64_t) * (size_t)B * (size_t)ahv::topk_modes_state_stride(N);   // the alive state: one key per hypothesis
}

int ahv_topk_modes_f32(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset, int K,
                       float min_trace, int64_t* keys, void* workspace, size_t workspace_bytes, void* stream)
{
    if (bad_k(K)) return fail(AHV_EINVAL, "topk_modes: K = %d outside 1..%d", K, AHV_TOPK_MAX_K);
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "topk_modes: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "topk_modes: B > 65535");
    if (n_offset < 0 || n_offset + N > 4294967296ll) return fail(AHV_EINVAL, "topk_modes: n_offset + N must fit in 32 bits");
    if (!(min_trace > -1.0f && min_trace < 3.0f))   // false for a NaN
        return fail(AHV_EINVAL, "topk_modes: min_trace = %g outside (-1, 3) (1 + 2 cos theta, 0 < theta < 180 degrees)",
                    (double)min_trace);
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "topk_modes: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (B == 0) return AHV_OK;
    if (!keys || (N > 0 && (!scores || !R))) return fail(AHV_EINVAL, "topk_modes: null pointer");
    const size_t need = ahv_topk_modes_workspace_bytes(B, N, K);
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return fail(AHV_EINVAL, "topk_modes: needs a 16-byte aligned workspace of %zu bytes (ahv_topk_modes_workspace_bytes), "
                    "got %zu", need, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {
        hipError_t e = ahv::launch_fill_keys(keys, B * K, s);
        if (e != hipSuccess) return hip_fail("topk_modes: list fill", e);
        return AHV_OK;
    }
    hipError_t e = ahv::launch_topk_modes(scores, R, r_batch_stride, B, N, n_offset, K, min_trace, keys,
                                          static_cast<int64_t*>(workspace), s);
    if (e != hipSuccess) return hip_fail("topk_modes: launch", e);
    return AHV_OK;
}

// ---- pose selection modulo a symmetry group ------------------------------------------------------------------
static int sym_group(const char* who, const float* S, int64_t s_batch_stride, int G, const float* axis, int64_t axis_batch_stride)
{
    if (G < 1 || G > AHV_SYM_MAX_ELEMENTS) return fail(AHV_EINVAL, "%s: G = %d outside 1..%d", who, G, AHV_SYM_MAX_ELEMENTS);
    if (s_batch_stride != 0 && s_batch_stride != (int64_t)G * 9)
        return fail(AHV_EINVAL, "%s: s_batch_stride %lld must be 0 or G*9", who, (long long)s_batch_stride);
    if (axis_batch_stride != 0 && axis_batch_stride != 3)
        return fail(AHV_EINVAL, "%s: axis_batch_stride %lld must be 0 or 3", who, (long long)axis_batch_stride);
    if (!S) return fail(AHV_EINVAL, "%s: null pointer (S)", who);
    (void)axis;
    return AHV_OK;
}

int ahv_topk_modes_sym_f32(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset, int K,
                           float min_trace, const float* S, int64_t s_batch_stride, int G, const float* axis,
                           int64_t axis_batch_stride, int64_t* keys, void* workspace, size_t workspace_bytes, void* stream)
{
    if (bad_k(K)) return fail(AHV_EINVAL, "topk_modes_sym: K = %d outside 1..%d", K, AHV_TOPK_MAX_K);
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "topk_modes_sym: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "topk_modes_sym: B > 65535");
    if (n_offset < 0 || n_offset + N > 4294967296ll) return fail(AHV_EINVAL, "topk_modes_sym: n_offset + N must fit in 32 bits");
    if (!(min_trace > -1.0f && min_trace < 3.0f))   // false for a NaN
        return fail(AHV_EINVAL, "topk_modes_sym: min_trace = %g outside (-1, 3) (1 + 2 cos theta, 0 < theta < 180 degrees)",
                    (double)min_trace);
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "topk_modes_sym: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (int rc = sym_group("topk_modes_sym", S, s_batch_stride, G, axis, axis_batch_stride)) return rc;
    if (B == 0) return AHV_OK;
    if (!keys || (N > 0 && (!scores || !R))) return fail(AHV_EINVAL, "topk_modes_sym: null pointer");
    const size_t need = ahv_topk_modes_workspace_bytes(B, N, K);
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return fail(AHV_EINVAL, "topk_modes_sym: needs a 16-byte aligned workspace of %zu bytes (ahv_topk_modes_workspace_bytes), "
                    "got %zu", need, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {
        hipError_t e = ahv::launch_fill_keys(keys, B * K, s);
        if (e != hipSuccess) return hip_fail("topk_modes_sym: list fill", e);
        return AHV_OK;
    }
    hipError_t e = ahv::launch_topk_modes_sym(scores, R, r_batch_stride, B, N, n_offset, K, min_trace, S, s_batch_stride, G, axis,
                                              axis_batch_stride, keys, static_cast<int64_t*>(workspace), s);
    if (e != hipSuccess) return hip_fail("topk_modes_sym: launch", e);
    return AHV_OK;
}

int ahv_sym_fold_f32(const float* R, int64_t r_batch_stride, int B, int64_t N, const float* S, int64_t s_batch_stride, int G,
                     const float* axis, int64_t axis_batch_stride, const float* anchors, int K, float min_trace, int64_t keep,
                     const float* V, float* R_out, float* V_out, int32_t* which, int32_t* elem, float* trace, void* stream)
{
    if (K < 1 || K > AHV_SYM_FOLD_MAX_ANCHORS) return fail(AHV_EINVAL, "sym_fold: K = %d outside 1..%d", K, AHV_SYM_FOLD_MAX_ANCHORS);
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "sym_fold: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "sym_fold: B > 65535");
    if (!(min_trace == -__builtin_inff() || (min_trace > -1.0f && min_trace < 3.0f)))   // false for a NaN
        return fail(AHV_EINVAL, "sym_fold: min_trace = %g is neither -inf (no limit) nor inside (-1, 3)", (double)min_trace);
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "sym_fold: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (int rc = sym_group("sym_fold", S, s_batch_stride, G, axis, axis_batch_stride)) return rc;
    if (keep < 0 || keep > N) return fail(AHV_EINVAL, "sym_fold: keep = %lld outside 0..N", (long long)keep);
    if ((V == nullptr) != (V_out == nullptr)) return fail(AHV_EINVAL, "sym_fold: V and V_out go together");
    if (B == 0 || N == 0) return AHV_OK;
    if (!R || !anchors || !R_out) return fail(AHV_EINVAL, "sym_fold: null pointer");
    hipError_t e = ahv::launch_sym_fold(R, r_batch_stride, B, N, S, s_batch_stride, G, axis, axis_batch_stride, anchors, K, min_trace,
                                        keep, V, R_out, V_out, which, elem, trace, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("sym_fold: launch", e);
    return AHV_OK;
}

// ---- multi-view verification ---------------------------------------------------------------------------------
static int views_sizes(const char* who, int B, int V, int64_t N)
{
    if (V < 1 || V > AHV_VIEWS_MAX) return fail(AHV_EINVAL, "%s: V = %d outside 1..%d", who, V, AHV_VIEWS_MAX);
    if (B < 1 || N < 1) return fail(AHV_EINVAL, "%s: B = %d and N = %lld must be at least 1", who, B, (long long)N);
    if (B > 65535) return fail(AHV_EINVAL, "%s: B > 65535", who);
    return AHV_OK;
}

// weights: V HOST floats or NULL (all ones)
static int views_weights(const char* who, const float* weights, int V)
{
    if (!weights) return AHV_OK;
    bool any = false;
    for (int v = 0; v < V; ++v) {
        if (!(weights[v] >= 0.0f && weights[v] < __builtin_inff()))   // false for a NaN
            return fail(AHV_EINVAL, "%s: weights[%d] = %g must be finite and >= 0", who, v, (double)weights[v]);
        any = any || weights[v] > 0.0f;
    }
    if (!any) return fail(AHV_EINVAL, "%s: weights are all zero (no view would take part)", who);
    return AHV_OK;
}

// the compact entries: the slot map is int32 and a list holds at most the whole set
static int views_compact_sizes(const char* who, int B, int V, int64_t N, int64_t capacity)
{
    if (int rc = views_sizes(who, B, V, N)) return rc;
    if (N >= (int64_t)1 << 31) return fail(AHV_EINVAL, "%s: N = %lld must be below 2^31 (the slot map is int32)", who, (long long)N);
    if (capacity < 1 || capacity > N)
        return fail(AHV_EINVAL, "%s: capacity = %lld outside 1..N = %lld", who, (long long)capacity, (long long)N);
    return AHV_OK;
}

int ahv_view_rotations_f32(const float* Q, int64_t q_batch_stride, const float* A, int B, int V, int64_t N, float* out,
                           void* stream)
{
    if (int rc = views_sizes("view_rotations", B, V, N)) return rc;
    if (N > 4294967296ll) return fail(AHV_EINVAL, "view_rotations: N must fit in 32 bits");
    if (q_batch_stride != 0 && q_batch_stride != N * 9)
        return fail(AHV_EINVAL, "view_rotations: q_batch_stride %lld must be 0 or N*9", (long long)q_batch_stride);
    if ((int64_t)B * V * N > (int64_t)1 << 38)
        return fail(AHV_EINVAL, "view_rotations: B*V*N = %lld output matrices exceed one launch (2^38)", (long long)((int64_t)B * V * N));
    if (!Q || !A || !out) return fail(AHV_EINVAL, "view_rotations: null pointer");
    hipError_t e = ahv::launch_view_rotations(Q, q_batch_stride, A, B, V, N, out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("view_rotations: launch", e);
    return AHV_OK;
}

int ahv_fuse_view_scores_f32(const float* scores, const float* Q, int64_t q_batch_stride, const float* A, const float* weights,
                             int B, int V, int64_t N, int64_t n_offset, float min_trace, float* fused, int64_t* best_key,
                             unsigned flags, void* stream)
{
    if (int rc = views_sizes("fuse_view_scores", B, V, N)) return rc;
    if (n_offset < 0 || n_offset + N > 4294967296ll)
        return fail(AHV_EINVAL, "fuse_view_scores: n_offset + N must fit in 32 bits");
    if (flags & ~(AHV_VIEWS_RESET_BEST | AHV_VIEWS_NO_ANGLE_LIMIT)) return fail(AHV_EINVAL, "fuse_view_scores: unknown flags 0x%x", flags);
    const bool limit = !(flags & AHV_VIEWS_NO_ANGLE_LIMIT);
    if (limit && !(min_trace > -1.0f && min_trace < 3.0f))   // false for a NaN
        return fail(AHV_EINVAL, "fuse_view_scores: min_trace = %g outside (-1, 3) (1 + 2 cos theta, 0 < theta < 180 degrees; "
                    "AHV_VIEWS_NO_ANGLE_LIMIT for none)", (double)min_trace);
    if (q_batch_stride != 0 && q_batch_stride != N * 9)
        return fail(AHV_EINVAL, "fuse_view_scores: q_batch_stride %lld must be 0 or N*9", (long long)q_batch_stride);
    if (!scores || !best_key || (limit && (!Q || !A))) return fail(AHV_EINVAL, "fuse_view_scores: null pointer");
    if (int rc = views_weights("fuse_view_scores", weights, V)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & AHV_VIEWS_RESET_BEST) {
        hipError_t e = ahv::launch_fill_keys(best_key, B, s);
        if (e != hipSuccess) return hip_fail("fuse_view_scores: key reset", e);
    }
    hipError_t e = ahv::launch_fuse_views(scores, Q, q_batch_stride, A, weights, B, V, N, n_offset, min_trace, limit, fused,
                                          best_key, s);
    if (e != hipSuccess) return hip_fail("fuse_view_scores: launch", e);
    return AHV_OK;
}

// the selection entries: K of V views per sample
static int views_selection(const char* who, int B, int V, int K)
{
    if (V < 1 || V > AHV_VIEWS_MAX) return fail(AHV_EINVAL, "%s: V = %d outside 1..%d", who, V, AHV_VIEWS_MAX);
    if (K < 1 || K > V) return fail(AHV_EINVAL, "%s: K = %d outside 1..V = %d", who, K, V);
    if (B < 1) return fail(AHV_EINVAL, "%s: B = %d must be at least 1", who, B);
    if (B > 65535) return fail(AHV_EINVAL, "%s: B > 65535", who);
    return AHV_OK;
}

int ahv_nearest_views_f32(const float* anchor, const float* A, int B, int V, int K, int32_t* view_idx, float* A_sel, void* stream)
{
    if (int rc = views_selection("nearest_views", B, V, K)) return rc;
    if (!anchor || !A || !view_idx || !A_sel) return fail(AHV_EINVAL, "nearest_views: null pointer");
    hipError_t e = ahv::launch_nearest_views(anchor, A, B, V, K, view_idx, A_sel, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("nearest_views: launch", e);
    return AHV_OK;
}

int ahv_gather_views_f32(const float* src, const int32_t* view_idx, int B, int V, int K, int64_t L, float* dst, unsigned flags,
                         void* stream)
{
    if (int rc = views_selection("gather_views", B, V, K)) return rc;
    if (flags & ~AHV_GATHER_BROADCAST) return fail(AHV_EINVAL, "gather_views: unknown flags 0x%x", flags);
    const bool broadcast = (flags & AHV_GATHER_BROADCAST) != 0;
    if (L < 4 || (L & 3)) return fail(AHV_EINVAL, "gather_views: L = %lld must be a positive multiple of 4 floats", (long long)L);
    if (L > (int64_t)1 << 40) return fail(AHV_EINVAL, "gather_views: L = %lld exceeds 2^40 floats per row", (long long)L);
    if (!src || !dst || (!broadcast && !view_idx)) return fail(AHV_EINVAL, "gather_views: null pointer");
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15)
        return fail(AHV_EINVAL, "gather_views: src and dst must be 16-byte aligned (the rows move as 16-byte words)");
    hipError_t e = ahv::launch_gather_views(src, view_idx, B, V, K, L / 4, dst, broadcast, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("gather_views: launch", e);
    return AHV_OK;
}

// ---- joint pose inference over an unposed image set --------------------------------------------------------------------
static int graph_sizes(const char* who, int B, int V)
{
    if (V < 2 || V > AHV_GRAPH_MAX_NODES) return fail(AHV_EINVAL, "%s: V = %d outside 2..%d", who, V, AHV_GRAPH_MAX_NODES);
    if (B < 1 || B > 65535) return fail(AHV_EINVAL, "%s: B = %d outside 1..65535", who, B);
    return AHV_OK;
}

static int graph_edges(const char* who, int E)
{
    if (E < 1 || E > AHV_GRAPH_MAX_EDGES) return fail(AHV_EINVAL, "%s: E = %d outside 1..%d", who, E, AHV_GRAPH_MAX_EDGES);
    return AHV_OK;
}

static int graph_node(const char* who, const char* what, int k, int V)
{
    if (k < 0 || k >= V) return fail(AHV_EINVAL, "%s: %s = %d outside 0..V-1 = %d", who, what, k, V - 1);
    return AHV_OK;
}

int ahv_pose_graph_init_f32(const float* pair_R, const float* pair_score, const int32_t* edges, int B, int V, int E, int root,
                            float* A, int32_t* parent_edge, int32_t* reached, void* stream)
{
    if (int rc = graph_sizes("pose_graph_init", B, V)) return rc;
    if (int rc = graph_edges("pose_graph_init", E)) return rc;
    if (int rc = graph_node("pose_graph_init", "root", root, V)) return rc;
    if (!pair_R || !pair_score || !edges || !A || !parent_edge || !reached) return fail(AHV_EINVAL, "pose_graph_init: null pointer");
    hipError_t e = ahv::launch_pose_graph_init(pair_R, pair_score, edges, B, V, E, root, A, parent_edge, reached,
                                               static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("pose_graph_init: launch", e);
    return AHV_OK;
}

int ahv_pose_graph_propose_f32(const float* A, const float* pair_R, const float* pair_score, const int32_t* edges,
                               const int32_t* incident, int B, int V, int E, int k, int D, int64_t N, int64_t n_fresh, uint64_t seed,
                               const int64_t* counter, int sweep, float sigma_rad, float* Q, float* Rrel, void* stream)
{
    if (int rc = graph_sizes("pose_graph_propose", B, V)) return rc;
    if (int rc = graph_edges("pose_graph_propose", E)) return rc;
    if (int rc = graph_node("pose_graph_propose", "k", k, V)) return rc;
    if (D < 1 || D > AHV_VIEWS_MAX)
        return fail(AHV_EINVAL, "pose_graph_propose: D = %d outside 1..%d (the fuse kernel takes the incident edges as its views)", D,
                    AHV_VIEWS_MAX);
    if (n_fresh < 0) return fail(AHV_EINVAL, "pose_graph_propose: n_fresh = %lld must be >= 0", (long long)n_fresh);
    if (N >= (int64_t)1 << 31) return fail(AHV_EINVAL, "pose_graph_propose: N = %lld must be below 2^31", (long long)N);
    if (n_fresh >= (int64_t)1 << 31 || N < 1 + D + n_fresh)
        return fail(AHV_EINVAL, "pose_graph_propose: N = %lld candidates do not hold 1 + D + n_fresh = %lld slots", (long long)N,
                    (long long)(1 + D + n_fresh));
    if (sweep < 0 || sweep > 255) return fail(AHV_EINVAL, "pose_graph_propose: sweep = %d outside 0..255", sweep);
    if (!(sigma_rad >= 0.0f && sigma_rad < __builtin_inff()))
        return fail(AHV_EINVAL, "pose_graph_propose: sigma = %g must be finite and >= 0", (double)sigma_rad);
    if (!A || !pair_R || !pair_score || !edges || !incident || !Q || !Rrel)
        return fail(AHV_EINVAL, "pose_graph_propose: null pointer (only counter may be NULL)");
    hipError_t e = ahv::launch_pose_graph_propose(A, pair_R, pair_score, edges, incident, B, V, E, k, D, N, n_fresh, seed, counter, sweep,
                                                  sigma_rad, Q, Rrel, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("pose_graph_propose: launch", e);
    return AHV_OK;
}

int ahv_pose_graph_commit_f32(const int64_t* key, const float* Q, int B, int V, int k, int64_t N, float* A, float* node_score,
                              void* stream)
{
    if (int rc = graph_sizes("pose_graph_commit", B, V)) return rc;
    if (int rc = graph_node("pose_graph_commit", "k", k, V)) return rc;
    if (N < 1 || N >= (int64_t)1 << 31) return fail(AHV_EINVAL, "pose_graph_commit: N = %lld outside 1..2^31-1", (long long)N);
    if (!key || !Q || !A || !node_score) return fail(AHV_EINVAL, "pose_graph_commit: null pointer");
    hipError_t e = ahv::launch_pose_graph_commit(key, Q, B, V, k, N, A, node_score, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("pose_graph_commit: launch", e);
    return AHV_OK;
}

size_t ahv_view_rotations_compact_workspace_bytes(int B, int V, int64_t N)
{
    if (B <= 0 || V < 1 || V > AHV_VIEWS_MAX || N <= 0) return 0;
    return sizeof(int32_t) * (size_t)B * (size_t)V * (size_t)ahv::view_compact_tiles(N);   // one count per (b, v, tile)
}

int ahv_view_rotations_compact_f32(const float* Q, int64_t q_batch_stride, const float* A, const float* weights, int B, int V,
                                   int64_t N, float min_trace, int64_t capacity, float* out, int32_t* slot, int64_t* counts,
                                   void* workspace, size_t workspace_bytes, void* stream)
{
    if (int rc = views_compact_sizes("view_rotations_compact", B, V, N, capacity)) return rc;
    if (!(min_trace > -1.0f && min_trace < 3.0f))   // false for a NaN
        return fail(AHV_EINVAL, "view_rotations_compact: min_trace = %g outside (-1, 3) (1 + 2 cos theta, 0 < theta < 180 degrees)",
                    (double)min_trace);
    if (q_batch_stride != 0 && q_batch_stride != N * 9)
        return fail(AHV_EINVAL, "view_rotations_compact: q_batch_stride %lld must be 0 or N*9", (long long)q_batch_stride);
    if (!Q || !A || !counts) return fail(AHV_EINVAL, "view_rotations_compact: null pointer");
    if (!out != !slot)
        return fail(AHV_EINVAL, "view_rotations_compact: out and slot must both be given, or both be NULL (count only)");
    if (int rc = views_weights("view_rotations_compact", weights, V)) return rc;
    const size_t need = ahv_view_rotations_compact_workspace_bytes(B, V, N);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 3))
        return fail(AHV_EINVAL, "view_rotations_compact: needs a 4-byte aligned workspace of %zu bytes "
                    "(ahv_view_rotations_compact_workspace_bytes), got %zu", need, workspace_bytes);
    hipError_t e = ahv::launch_view_rotations_compact(Q, q_batch_stride, A, weights, B, V, N, min_trace, capacity, out, slot, counts,
                                                      workspace, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("view_rotations_compact: launch", e);
    return AHV_OK;
}

int ahv_fuse_view_scores_compact_f32(const float* scores, const int32_t* slot, const float* weights, int B, int V, int64_t N,
                                     int64_t capacity, int64_t n_offset, float* fused, int64_t* best_key, unsigned flags,
                                     void* stream)
{
    if (int rc = views_compact_sizes("fuse_view_scores_compact", B, V, N, capacity)) return rc;
    if (n_offset < 0 || n_offset + N > 4294967296ll)
        return fail(AHV_EINVAL, "fuse_view_scores_compact: n_offset + N must fit in 32 bits");
    if (flags & ~AHV_VIEWS_RESET_BEST) return fail(AHV_EINVAL, "fuse_view_scores_compact: unknown flags 0x%x", flags);
    if (!scores || !slot || !best_key) return fail(AHV_EINVAL, "fuse_view_scores_compact: null pointer");
    if (int rc = views_weights("fuse_view_scores_compact", weights, V)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & AHV_VIEWS_RESET_BEST) {
        hipError_t e = ahv::launch_fill_keys(best_key, B, s);
        if (e != hipSuccess) return hip_fail("fuse_view_scores_compact: key reset", e);
    }
    hipError_t e = ahv::launch_fuse_views_compact(scores, slot, weights, B, V, N, capacity, n_offset, fused, best_key, s);
    if (e != hipSuccess) return hip_fail("fuse_view_scores_compact: launch", e);
    return AHV_OK;
}

// ---- pose posterior ----------------------------------------------------------------------------------------
static bool bad_modes(int K) { return K < 0 || K > AHV_POSTERIOR_MAX_MODES; }
static bool bad_beta(float beta) { return !(beta > 0.0f && beta < __builtin_inff()); }   // false for a NaN

size_t ahv_pose_posterior_state_bytes(int B, int K)
{
    if (B <= 0 || bad_modes(K)) return 0;
    return (size_t)B * ahv::posterior_state_stride(K);
}

size_t ahv_pose_posterior_workspace_bytes(int B, int64_t N, int K)
{
    if (B <= 0 || N <= 0 || bad_modes(K)) return 0;
    return (size_t)ahv::posterior_parts(N) * (size_t)B * ahv::posterior_state_stride(K);   // one partial state per workgroup
}

int ahv_pose_posterior_f32(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, const float* anchors,
                           int K, float min_trace, float beta, void* state, void* workspace, size_t workspace_bytes,
                           unsigned flags, void* stream)
{
    if (bad_modes(K)) return fail(AHV_EINVAL, "pose_posterior: K = %d outside 0..%d", K, AHV_POSTERIOR_MAX_MODES);
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "pose_posterior: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "pose_posterior: B > 65535");
    if (bad_beta(beta)) return fail(AHV_EINVAL, "pose_posterior: beta = %g must be finite and > 0 (1 / temperature)", (double)beta);
    if (!(min_trace > -1.0f && min_trace < 3.0f))   // false for a NaN
        return fail(AHV_EINVAL, "pose_posterior: min_trace = %g outside (-1, 3) (1 + 2 cos theta, 0 < theta < 180 degrees)",
                    (double)min_trace);
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "pose_posterior: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (flags & ~AHV_POSTERIOR_RESET_STATE) return fail(AHV_EINVAL, "pose_posterior: unknown flags 0x%x", flags);
    if (B == 0) return AHV_OK;
    if (!state || (N > 0 && (!scores || !R)) || (K > 0 && N > 0 && !anchors)) return fail(AHV_EINVAL, "pose_posterior: null pointer");
    if (reinterpret_cast<uintptr_t>(state) & 15) return fail(AHV_EINVAL, "pose_posterior: state must be 16-byte aligned");
    const size_t need = ahv_pose_posterior_workspace_bytes(B, N, K);
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return fail(AHV_EINVAL, "pose_posterior: needs a 16-byte aligned workspace of %zu bytes (ahv_pose_posterior_workspace_bytes), "
                    "got %zu", need, workspace_bytes);
    const bool reset = (flags & AHV_POSTERIOR_RESET_STATE) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {
        if (!reset) return AHV_OK;
        hipError_t e = ahv::launch_posterior_merge(nullptr, 0, B, K, beta, state, false, s);   // an empty state
        if (e != hipSuccess) return hip_fail("pose_posterior: state reset", e);
        return AHV_OK;
    }
    hipError_t e = ahv::launch_posterior(scores, R, r_batch_stride, B, N, anchors, K, min_trace, beta, state, workspace, !reset, s);
    if (e != hipSuccess) return hip_fail("pose_posterior: launch", e);
    return AHV_OK;
}

int ahv_pose_posterior_merge(const void* states, int P, int B, int K, float beta, void* state, unsigned flags, void* stream)
{
    if (bad_modes(K)) return fail(AHV_EINVAL, "pose_posterior_merge: K = %d outside 0..%d", K, AHV_POSTERIOR_MAX_MODES);
    if (B < 0 || P < 0) return fail(AHV_EINVAL, "pose_posterior_merge: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "pose_posterior_merge: B > 65535");
    if (bad_beta(beta)) return fail(AHV_EINVAL, "pose_posterior_merge: beta = %g must be finite and > 0 (1 / temperature)", (double)beta);
    if (flags & ~AHV_POSTERIOR_RESET_STATE) return fail(AHV_EINVAL, "pose_posterior_merge: unknown flags 0x%x", flags);
    if (B == 0) return AHV_OK;
    if (!state || (P > 0 && !states)) return fail(AHV_EINVAL, "pose_posterior_merge: null pointer");
    if ((reinterpret_cast<uintptr_t>(state) & 15) || (reinterpret_cast<uintptr_t>(states) & 15))
        return fail(AHV_EINVAL, "pose_posterior_merge: states must be 16-byte aligned");
    const bool reset = (flags & AHV_POSTERIOR_RESET_STATE) != 0;
    if (P == 0 && !reset) return AHV_OK;
    hipError_t e = ahv::launch_posterior_merge(states, P, B, K, beta, state, !reset, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("pose_posterior_merge: launch", e);
    return AHV_OK;
}

int ahv_pose_posterior_finish_f32(const void* state, int B, int K, float beta, float* log_z, float* entropy, float* mean_score,
                                  int64_t* n_excluded, float* mode_prob, float* rest_prob, float* mode_R_mean, float* R_mean,
                                  float* mode_spread_deg, float* spread_deg, void* stream)
{
    if (bad_modes(K)) return fail(AHV_EINVAL, "pose_posterior_finish: K = %d outside 0..%d", K, AHV_POSTERIOR_MAX_MODES);
    if (B < 0) return fail(AHV_EINVAL, "pose_posterior_finish: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "pose_posterior_finish: B > 65535");
    if (bad_beta(beta)) return fail(AHV_EINVAL, "pose_posterior_finish: beta = %g must be finite and > 0 (1 / temperature)", (double)beta);
    if (B == 0) return AHV_OK;
    if (!state) return fail(AHV_EINVAL, "pose_posterior_finish: null state");
    if (reinterpret_cast<uintptr_t>(state) & 15) return fail(AHV_EINVAL, "pose_posterior_finish: state must be 16-byte aligned");
    hipError_t e = ahv::launch_posterior_finish(state, B, K, beta, log_z, entropy, mean_score, n_excluded, mode_prob, rest_prob,
                                                mode_R_mean, R_mean, mode_spread_deg, spread_deg, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("pose_posterior_finish: launch", e);
    return AHV_OK;
}

// ---- posterior resampling ------------------------------------------------------------------------------------
size_t ahv_resample_workspace_bytes(int B, int64_t N)
{
    if (B <= 0 || N <= 0 || N > 4294967296ll) return 0;
    return (size_t)B * ahv::resample_stride(N);   // per sample a 32-byte header and one 16-byte record per tile, plus one
}

int ahv_resample_f32(const float* scores, int B, int64_t N, float beta, int64_t M, const float* u, int64_t* idx, void* workspace,
                     size_t workspace_bytes, unsigned flags, void* stream)
{
    if (B < 0) return fail(AHV_EINVAL, "resample: negative size");
    if (B > 65535) return fail(AHV_EINVAL, "resample: B > 65535");
    if (N < 1 || N > 4294967296ll) return fail(AHV_EINVAL, "resample: N = %lld outside 1..2^32", (long long)N);
    if (M < 1 || M >= (int64_t)1 << 31) return fail(AHV_EINVAL, "resample: M = %lld outside 1..2^31-1", (long long)M);
    if (bad_beta(beta)) return fail(AHV_EINVAL, "resample: beta = %g must be finite and > 0 (1 / temperature)", (double)beta);
    if (flags) return fail(AHV_EINVAL, "resample: unknown flags 0x%x", flags);
    if (B == 0) return AHV_OK;
    if (!scores || !idx) return fail(AHV_EINVAL, "resample: null pointer");
    const size_t need = ahv_resample_workspace_bytes(B, N);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(AHV_EINVAL, "resample: needs a 16-byte aligned workspace of %zu bytes (ahv_resample_workspace_bytes), got %zu",
                    need, workspace_bytes);
    hipError_t e = ahv::launch_resample(scores, B, N, beta, M, u, idx, workspace, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("resample: launch", e);
    return AHV_OK;
}

int ahv_compose_rotations_indexed_f32(const int64_t* idx, const float* R, int64_t r_batch_stride, int64_t N, const float* D,
                                      int64_t M, int B, float* out, void* stream)
{
    if (B < 0 || N < 0 || M < 0) return fail(AHV_EINVAL, "compose_rotations_indexed: negative size");
    if ((int64_t)B * M > (int64_t)1 << 38)
        return fail(AHV_EINVAL, "compose_rotations_indexed: B*M = %lld output matrices exceed one launch (2^38)",
                    (long long)((int64_t)B * M));
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "compose_rotations_indexed: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (B == 0 || M == 0) return AHV_OK;
    if (!idx || !R || !D || !out) return fail(AHV_EINVAL, "compose_rotations_indexed: null pointer");
    if (N == 0) return fail(AHV_EINVAL, "compose_rotations_indexed: empty rotation set");
    hipError_t e = ahv::launch_compose_rotations_indexed(idx, R, r_batch_stride, N, D, M, B, out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("compose_rotations_indexed: launch", e);
    return AHV_OK;
}

// ---- pose tracking: the predict step and the start of a step ----------------------------------------------------
int ahv_diffuse_rotations_f32(const int64_t* idx, const float* R, int64_t r_batch_stride, int64_t N, const int64_t* best_key,
                              int64_t M, int64_t n_fresh, int B, uint64_t seed, const int64_t* step, float sigma_rad,
                              float max_angle_rad, float* out, float* omega, void* stream)
{
    if (!R || !out || !step) return fail(AHV_EINVAL, "diffuse_rotations: null pointer (R, out and step are required)");
    if (M < 1 || M >= (int64_t)1 << 31) return fail(AHV_EINVAL, "diffuse_rotations: M = %lld outside 1..2^31-1", (long long)M);
    if (N < 1) return fail(AHV_EINVAL, "diffuse_rotations: empty rotation set (N = %lld)", (long long)N);
    if (n_fresh < 0 || n_fresh > M)
        return fail(AHV_EINVAL, "diffuse_rotations: n_fresh = %lld outside 0..M = %lld", (long long)n_fresh, (long long)M);
    if (B < 1 || B > 65535) return fail(AHV_EINVAL, "diffuse_rotations: B = %d outside 1..65535", B);
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "diffuse_rotations: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (!(sigma_rad >= 0.0f && sigma_rad < __builtin_inff()))
        return fail(AHV_EINVAL, "diffuse_rotations: sigma = %g must be finite and >= 0", (double)sigma_rad);
    if (!(max_angle_rad >= 0.0f && max_angle_rad < __builtin_inff()))
        return fail(AHV_EINVAL, "diffuse_rotations: max_angle = %g must be finite and >= 0 (0: no limit)", (double)max_angle_rad);
    hipError_t e = ahv::launch_diffuse_rotations(idx, R, r_batch_stride, N, best_key, M, n_fresh, B, seed, step, sigma_rad,
                                                 max_angle_rad, out, omega, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("diffuse_rotations: launch", e);
    return AHV_OK;
}

int ahv_predict_rotations_f32(const int64_t* idx, const float* R, int64_t r_batch_stride, const float* V, int64_t v_batch_stride,
                              int64_t N, const int64_t* best_key, int64_t M, int64_t n_fresh, int B, uint64_t seed,
                              const int64_t* step, float sigma_rad, float sigma_vel_rad, float damping, float max_angle_rad,
                              float max_speed_rad, int coast, float* out, float* vel_out, float* omega, void* stream)
{
    const auto angle = [](float a) { return a >= 0.0f && a < __builtin_inff(); };
    if (!R || !out || !vel_out || !step)
        return fail(AHV_EINVAL, "predict_rotations: null pointer (R, out, vel_out and step are required)");
    if (M < 1 || M >= (int64_t)1 << 31) return fail(AHV_EINVAL, "predict_rotations: M = %lld outside 1..2^31-1", (long long)M);
    if (N < 1) return fail(AHV_EINVAL, "predict_rotations: empty rotation set (N = %lld)", (long long)N);
    if (n_fresh < 0 || n_fresh > M)
        return fail(AHV_EINVAL, "predict_rotations: n_fresh = %lld outside 0..M = %lld", (long long)n_fresh, (long long)M);
    if (B < 1 || B > 65535) return fail(AHV_EINVAL, "predict_rotations: B = %d outside 1..65535", B);
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "predict_rotations: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (v_batch_stride != 0 && v_batch_stride != N * 3)
        return fail(AHV_EINVAL, "predict_rotations: v_batch_stride %lld must be 0 or N*3", (long long)v_batch_stride);
    if (!angle(sigma_rad)) return fail(AHV_EINVAL, "predict_rotations: sigma = %g must be finite and >= 0", (double)sigma_rad);
    if (!angle(sigma_vel_rad))
        return fail(AHV_EINVAL, "predict_rotations: sigma_vel = %g must be finite and >= 0", (double)sigma_vel_rad);
    if (!(damping >= 0.0f && damping <= 1.0f))
        return fail(AHV_EINVAL, "predict_rotations: damping = %g outside [0, 1]", (double)damping);
    if (!angle(max_angle_rad))
        return fail(AHV_EINVAL, "predict_rotations: max_angle = %g must be finite and >= 0 (0: no limit)", (double)max_angle_rad);
    if (!angle(max_speed_rad))
        return fail(AHV_EINVAL, "predict_rotations: max_speed = %g must be finite and >= 0 (0: no limit)", (double)max_speed_rad);
    hipError_t e = ahv::launch_predict_rotations(idx, R, r_batch_stride, V, v_batch_stride, N, best_key, M, n_fresh, B, seed, step,
                                                 sigma_rad, sigma_vel_rad, damping, max_angle_rad, max_speed_rad, coast != 0, out,
                                                 vel_out, omega, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("predict_rotations: launch", e);
    return AHV_OK;
}

int ahv_track_advance(uint64_t seed, int64_t* step, int B, float* u, void* stream)
{
    if (!step || !u) return fail(AHV_EINVAL, "track_advance: null pointer");
    if (B < 1 || B > 65535) return fail(AHV_EINVAL, "track_advance: B = %d outside 1..65535", B);
    hipError_t e = ahv::launch_track_advance(seed, step, B, u, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("track_advance: launch", e);
    return AHV_OK;
}

// ---- pose tracking: noise scale and fresh slots adapted on the device ----------------------------------------------
static_assert(AHV_TRACK_CONTROL_WORDS == 8, "ahv_track.hip lays the control record out as eight words");

int ahv_predict_rotations_ctl_f32(const int64_t* idx, const float* R, int64_t r_batch_stride, const float* V, int64_t v_batch_stride,
                                  int64_t N, const int64_t* best_key, int64_t M, const uint32_t* control, int B, uint64_t seed,
                                  const int64_t* step, float damping, float max_angle_rad, float max_speed_rad, int coast,
                                  float* out, float* vel_out, float* omega, void* stream)
{
    const auto angle = [](float a) { return a >= 0.0f && a < __builtin_inff(); };
    if (!R || !out || !step || !control)
        return fail(AHV_EINVAL, "predict_rotations_ctl: null pointer (R, out, step and control are required)");
    if (!vel_out && (V || coast != 0))
        return fail(AHV_EINVAL, "predict_rotations_ctl: vel_out is required with V or a coast slot (without all three: the walk)");
    if (M < 1 || M >= (int64_t)1 << 31) return fail(AHV_EINVAL, "predict_rotations_ctl: M = %lld outside 1..2^31-1", (long long)M);
    if (N < 1) return fail(AHV_EINVAL, "predict_rotations_ctl: empty rotation set (N = %lld)", (long long)N);
    if (B < 1 || B > 65535) return fail(AHV_EINVAL, "predict_rotations_ctl: B = %d outside 1..65535", B);
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "predict_rotations_ctl: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (v_batch_stride != 0 && v_batch_stride != N * 3)
        return fail(AHV_EINVAL, "predict_rotations_ctl: v_batch_stride %lld must be 0 or N*3", (long long)v_batch_stride);
    if (!(damping >= 0.0f && damping <= 1.0f))
        return fail(AHV_EINVAL, "predict_rotations_ctl: damping = %g outside [0, 1]", (double)damping);
    if (!angle(max_angle_rad))
        return fail(AHV_EINVAL, "predict_rotations_ctl: max_angle = %g must be finite and >= 0 (0: no limit)", (double)max_angle_rad);
    if (!angle(max_speed_rad))
        return fail(AHV_EINVAL, "predict_rotations_ctl: max_speed = %g must be finite and >= 0 (0: no limit)", (double)max_speed_rad);
    hipError_t e = ahv::launch_predict_rotations_ctl(idx, R, r_batch_stride, V, v_batch_stride, N, best_key, M, control, B, seed, step,
                                                     damping, max_angle_rad, max_speed_rad, coast != 0, out, vel_out, omega,
                                                     static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("predict_rotations_ctl: launch", e);
    return AHV_OK;
}

int ahv_track_control_f32(const float* R_cur, const float* V_cur, const int64_t* idx, const float* score, int B, int64_t M, int first,
                          float sigma0_rad, float sigma_vel0_rad, int64_t n_fresh0, float sigma_min_rad, float sigma_max_rad,
                          float gain, float rate, float score_floor, int64_t n_fresh_lost, uint32_t* control, uint8_t* reacquired,
                          void* stream)
{
    const auto positive = [](float a) { return a > 0.0f && a < __builtin_inff(); };
    if (!R_cur || !idx || !score || !control || !reacquired)
        return fail(AHV_EINVAL, "track_control: null pointer (R_cur, idx, score, control and reacquired are required)");
    if (M < 1 || M >= (int64_t)1 << 31) return fail(AHV_EINVAL, "track_control: M = %lld outside 1..2^31-1", (long long)M);
    if (B < 1 || B > 65535) return fail(AHV_EINVAL, "track_control: B = %d outside 1..65535", B);
    if (first != 1 && first != 2) return fail(AHV_EINVAL, "track_control: first = %d must be 1, or 2 with a coast slot", first);
    if (!positive(sigma_min_rad) || !positive(sigma_max_rad) || sigma_min_rad > sigma_max_rad)
        return fail(AHV_EINVAL, "track_control: sigma_min = %g and sigma_max = %g must be finite with 0 < sigma_min <= sigma_max",
                    (double)sigma_min_rad, (double)sigma_max_rad);
    if (!positive(sigma0_rad)) return fail(AHV_EINVAL, "track_control: sigma0 = %g must be finite and > 0", (double)sigma0_rad);
    if (!(sigma_vel0_rad >= 0.0f && sigma_vel0_rad < __builtin_inff()))
        return fail(AHV_EINVAL, "track_control: sigma_vel0 = %g must be finite and >= 0", (double)sigma_vel0_rad);
    if (!positive(gain)) return fail(AHV_EINVAL, "track_control: gain = %g must be finite and > 0", (double)gain);
    if (!(rate > 0.0f && rate <= 1.0f)) return fail(AHV_EINVAL, "track_control: rate = %g outside (0, 1]", (double)rate);
    if (score_floor != score_floor) return fail(AHV_EINVAL, "track_control: score_floor is NaN (-inf: no floor)");
    if (n_fresh0 < 0 || n_fresh0 > M)
        return fail(AHV_EINVAL, "track_control: n_fresh0 = %lld outside 0..M = %lld", (long long)n_fresh0, (long long)M);
    if (n_fresh_lost < 0 || n_fresh_lost > M)
        return fail(AHV_EINVAL, "track_control: n_fresh_lost = %lld outside 0..M = %lld", (long long)n_fresh_lost, (long long)M);
    hipError_t e = ahv::launch_track_control(R_cur, V_cur, idx, score, B, M, first, sigma0_rad, sigma_vel0_rad, (int)n_fresh0,
                                             sigma_min_rad, sigma_max_rad, gain, rate, score_floor, (int)n_fresh_lost, control,
                                             reacquired, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("track_control: launch", e);
    return AHV_OK;
}

// ---- pose tracking: trajectory smoothing over the particle history ---------------------------------------------------
static int smooth_sizes(const char* who, int B, int64_t M, int64_t H)
{
    if (M < 1 || M >= (int64_t)1 << 31) return fail(AHV_EINVAL, "%s: M = %lld outside 1..2^31-1", who, (long long)M);
    if (B < 1 || B > 65535) return fail(AHV_EINVAL, "%s: B = %d outside 1..65535", who, B);
    if (H < 2 || H >= (int64_t)1 << 31) return fail(AHV_EINVAL, "%s: H = %lld outside 2..2^31-1", who, (long long)H);
    return AHV_OK;
}

int ahv_smooth_step_f32(const float* R_cur, const float* scores, const float* V_cur, const int64_t* step, int64_t first_step, int B,
                        int64_t M, int64_t H, float beta, float sigma_rad, float jump, float damping, float* hist_R, float* hist_P,
                        float* hist_delta, int32_t* hist_back, void* stream)
{
    if (int rc = smooth_sizes("smooth_step", B, M, H)) return rc;
    if (!R_cur || !scores || !step || !hist_R || !hist_delta || !hist_back)
        return fail(AHV_EINVAL, "smooth_step: null pointer (R_cur, scores, step, hist_R, hist_delta and hist_back are required)");
    if ((V_cur != nullptr) != (hist_P != nullptr))
        return fail(AHV_EINVAL, "smooth_step: V_cur and hist_P go together (both or neither)");
    if (!(beta > 0.0f && beta < __builtin_inff())) return fail(AHV_EINVAL, "smooth_step: beta = %g must be finite and > 0", (double)beta);
    // 1 / (4 sigma^2) is the kernel's factor: it has to fit a float
    const double inv4s2 = 1.0 / (4.0 * (double)sigma_rad * (double)sigma_rad);
    if (!(sigma_rad > 0.0f && sigma_rad < __builtin_inff() && inv4s2 < 3.0e38))
        return fail(AHV_EINVAL, "smooth_step: sigma = %g must be finite and > 0, with 1/(4 sigma^2) inside a float", (double)sigma_rad);
    if (!(jump >= 0.0f)) return fail(AHV_EINVAL, "smooth_step: jump = %g must be >= 0 (+inf: no floor)", (double)jump);
    if (!(damping >= 0.0f && damping <= 1.0f)) return fail(AHV_EINVAL, "smooth_step: damping = %g outside [0, 1]", (double)damping);
    hipError_t e = ahv::launch_smooth_step(R_cur, scores, V_cur, step, first_step, B, M, H, beta, (float)inv4s2, jump, damping, hist_R,
                                           hist_P, hist_delta, hist_back, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("smooth_step: launch", e);
    return AHV_OK;
}

int ahv_smooth_backtrace_f32(const float* hist_R, const float* hist_delta, const int32_t* hist_back, const int64_t* step,
                             int64_t first_step, int B, int64_t M, int64_t H, int64_t F, int64_t* path_idx, float* path_R,
                             void* stream)
{
    if (int rc = smooth_sizes("smooth_backtrace", B, M, H)) return rc;
    if (F < 1 || F > H) return fail(AHV_EINVAL, "smooth_backtrace: F = %lld outside 1..H = %lld", (long long)F, (long long)H);
    if (!hist_R || !hist_delta || !hist_back || !step || !path_idx || !path_R) return fail(AHV_EINVAL, "smooth_backtrace: null pointer");
    hipError_t e = ahv::launch_smooth_backtrace(hist_R, hist_delta, hist_back, step, first_step, B, M, H, F, path_idx, path_R,
                                                static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("smooth_backtrace: launch", e);
    return AHV_OK;
}

// ---- pose tracking: forward-backward marginal smoothing over the same ring --------------------------------------------
// sigma and jump as ahv_smooth_step_f32 checks them; *inv4s2 is the kernels' factor.
static int marginal_transition(const char* who, float sigma_rad, float jump, float* inv4s2)
{
    const double k = 1.0 / (4.0 * (double)sigma_rad * (double)sigma_rad);
    if (!(sigma_rad > 0.0f && sigma_rad < __builtin_inff() && k < 3.0e38))
        return fail(AHV_EINVAL, "%s: sigma = %g must be finite and > 0, with 1/(4 sigma^2) inside a float", who, (double)sigma_rad);
    if (!(jump >= 0.0f)) return fail(AHV_EINVAL, "%s: jump = %g must be >= 0 (+inf: no floor)", who, (double)jump);
    *inv4s2 = (float)k;
    return AHV_OK;
}

int ahv_marginal_step_f32(const float* R_cur, const float* scores, const int64_t* step, int64_t first_step, int B, int64_t M,
                          int64_t H, float beta, float sigma_rad, float jump, const float* hist_R, const float* hist_P,
                          float* hist_alpha, float* hist_emit, void* stream)
{
    if (int rc = smooth_sizes("marginal_step", B, M, H)) return rc;
    if (!R_cur || !scores || !step || !hist_R || !hist_alpha || !hist_emit)
        return fail(AHV_EINVAL, "marginal_step: null pointer (R_cur, scores, step, hist_R, hist_alpha and hist_emit are required)");
    if (!(beta > 0.0f && beta < __builtin_inff())) return fail(AHV_EINVAL, "marginal_step: beta = %g must be finite and > 0", (double)beta);
    float inv4s2;
    if (int rc = marginal_transition("marginal_step", sigma_rad, jump, &inv4s2)) return rc;
    hipError_t e = ahv::launch_marginal_step(R_cur, scores, step, first_step, B, M, H, beta, inv4s2, jump, hist_R, hist_P, hist_alpha,
                                             hist_emit, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("marginal_step: launch", e);
    return AHV_OK;
}

int ahv_marginal_smooth_f32(const float* hist_R, const float* hist_P, const float* hist_alpha, const float* hist_emit,
                            const int64_t* step, int64_t first_step, int B, int64_t M, int64_t H, int64_t F, float sigma_rad,
                            float jump, float* logw, int64_t* idx, float* R, void* stream)
{
    if (int rc = smooth_sizes("marginal_smooth", B, M, H)) return rc;
    if (F < 1 || F > H) return fail(AHV_EINVAL, "marginal_smooth: F = %lld outside 1..H = %lld", (long long)F, (long long)H);
    if (!hist_R || !hist_alpha || !hist_emit || !step || !logw || !idx || !R)
        return fail(AHV_EINVAL, "marginal_smooth: null pointer (only hist_P may be NULL)");
    float inv4s2;
    if (int rc = marginal_transition("marginal_smooth", sigma_rad, jump, &inv4s2)) return rc;
    hipError_t e = ahv::launch_marginal_smooth(hist_R, hist_P, hist_alpha, hist_emit, step, first_step, B, M, H, F, inv4s2, jump, logw,
                                               idx, R, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("marginal_smooth: launch", e);
    return AHV_OK;
}

// ---- rotation gradient of the score, SO(3) ascent step -------------------------------------------------
size_t ahv_score_rotation_grad_workspace_bytes(int B, int64_t N)
{
    if (B <= 0 || N <= 0) return 0;
    return sizeof(float) * 2048 * (size_t)B * (size_t)N;   // dL/du of every hypothesis
}

int ahv_score_rotation_grad_f32(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                const float* W1, const float* W2, const float* b2, int B, int64_t N,
                                const float* grad_scores, void* workspace, size_t workspace_bytes, float* grad_R,
                                void* stream)
{
    if (B < 0 || N < 0) return fail(AHV_EINVAL, "score_rotation_grad: negative size (B=%d, N=%lld)", B, (long long)N);
    if (B == 0 || N == 0) return AHV_OK;
    if (!vol_src || !feat_tgt || !R || !W1 || !W2 || !b2 || !grad_R || !workspace)
        return fail(AHV_EINVAL, "score_rotation_grad: null pointer");
    if (r_batch_stride != 0 && r_batch_stride != N * 9)
        return fail(AHV_EINVAL, "score_rotation_grad: r_batch_stride %lld must be 0 or N*9", (long long)r_batch_stride);
    if (workspace_bytes < ahv_score_rotation_grad_workspace_bytes(B, N))
        return fail(AHV_EINVAL, "score_rotation_grad: workspace of %zu bytes, need %zu (ahv_score_rotation_grad_workspace_bytes)",
                    workspace_bytes, ahv_score_rotation_grad_workspace_bytes(B, N));
    if (reinterpret_cast<uintptr_t>(workspace) & 15)
        return fail(AHV_EINVAL, "score_rotation_grad: workspace must be 16-byte aligned");
    const int cu = cu_count();
    if (cu <= 0) return fail(AHV_EDEVICE, "score_rotation_grad: no usable HIP device");
    hipError_t e = ahv::launch_score_rotation_grad(vol_src, feat_tgt, R, r_batch_stride, W1, W2, b2, B, N, grad_scores,
                                                   static_cast<float*>(workspace), grad_R, cu, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("score_rotation_grad: launch", e);
    return AHV_OK;
}

static int so3_ascent_sizes(const char* who, int L, int B, int K)
{
    if (L < 1 || L > AHV_SO3_MAX_LADDER) return fail(AHV_EINVAL, "%s: L = %d outside 1..%d", who, L, AHV_SO3_MAX_LADDER);
    if (bad_k(K)) return fail(AHV_EINVAL, "%s: K = %d outside 1..%d", who, K, AHV_TOPK_MAX_K);
    if (B < 0) return fail(AHV_EINVAL, "%s: negative size", who);
    if (B > 65535) return fail(AHV_EINVAL, "%s: B > 65535", who);   // B * K stays far inside an int
    return AHV_OK;
}

int ahv_so3_ascent_candidates_f32(const float* R_cur, const float* grad_R, const float* theta, const float* ladder, int L,
                                  int B, int K, float* R_cand, void* stream)
{
    if (int rc = so3_ascent_sizes("so3_ascent_candidates", L, B, K)) return rc;
    if (B == 0) return AHV_OK;
    if (!R_cur || !grad_R || !theta || !ladder || !R_cand) return fail(AHV_EINVAL, "so3_ascent_candidates: null pointer");
    hipError_t e = ahv::launch_so3_ascent_candidates(R_cur, grad_R, theta, ladder, L, B, K, R_cand,
                                                     static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("so3_ascent_candidates: launch", e);
    return AHV_OK;
}

int ahv_so3_ascent_select_f32(const float* R_cand, const float* cand_scores, const float* ladder, int L, int B, int K,
                              float* R_cur, float* score_cur, float* theta, void* stream)
{
    if (int rc = so3_ascent_sizes("so3_ascent_select", L, B, K)) return rc;
    if (B == 0) return AHV_OK;
    if (!R_cand || !cand_scores || !ladder || !R_cur || !score_cur || !theta)
        return fail(AHV_EINVAL, "so3_ascent_select: null pointer");
    hipError_t e = ahv::launch_so3_ascent_select(R_cand, cand_scores, ladder, L, B, K, R_cur, score_cur, theta,
                                                 static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail("so3_ascent_select: launch", e);
    return AHV_OK;
}

}  // extern "C"
