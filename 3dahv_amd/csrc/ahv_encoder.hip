// ahv_encoder.hip -- host side of the reference's "3D-aware encoder" on HIP kernels
// (transformer/attention.py: BasicTransformerBlock :240-258, CrossAttention :196-237, FeedForward/GEGLU
// :81-108, BidirectionTransformerBlock :260-274; Feature_Aligner.forward_2d3d, modules/modules.py:86-101).
// Once per image pair; 64 tokens x 256 channels per stream, so at small batches every GEMM is "skinny"
// (M = 64*B rows): its cost is streaming the weights once and the launch count.  The two streams of a layer
// (self_1 | self_2, then cross_1 | cross_2) are independent, so every launch carries BOTH blocks (and, for
// cross-attention, both the q and the k|v projections) as separate "problems": 6 launches per half layer, 48
// for the whole depth-4 encoder.
//
//   ahv_enc_linear.h   linear_staged_kernel, linear_kernel (3-D taps), linear_tile_kernel
//   ahv_enc_rows.h     attention_heads_kernel, attention_sample_head_kernel, ln_kernel, the kernels around the token stage
//   ahv_enc_probe.h    AHV_ENC_LAUNCH and the in-kernel stamps of tools/kbench_enc.cpp
//   ahv_enc_plan.h     which of them a launch takes at a batch size, and the workspace layouts (no HIP: tested on the CPU)
//
// One translation unit: the tools include this file as a whole.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ahv.h"
#include "ahv_launch.h"
#include "ahv_enc_plan.h"
#include "ahv_enc_linear.h"
#include "ahv_enc_rows.h"

namespace ahv {

// ---- host side -------------------------------------------------------------------------------------
struct LinSpec {
    const float* X;
    const float* W;
    float* P;
    const float* bias;
    int N;
};

// K axis of an implicit-GEMM convolution: (tap, channel)
enum TapMode { kTapNone = 0, kTap2d = 1, kTap3d = 2 };

static constexpr int lin_key(int k, bool geglu, int taps) { return k * 8 + (int)geglu * 4 + taps; }

// Every linear of the encoder: `nprob` problems X[M][ldx] . W[N][ldw]^T over K, split KS ways into slabs P[ks][M][N]
// (geglu_h = H > 0: one slice, W has 2H rows, bias + GEGLU epilogue, output [M][H]).  The form comes from the caller's plan
// (ahv_enc_plan.h); within the form, (K per slice | tile size, GEGLU, tap mode) names the instantiation in the table below,
// and anything outside it is an error.
static hipError_t launch_linear(LinForm form, const LinSpec* specs, int nprob, long ldx, long ldw, int M, int K, int KS,
                                int geglu_h, hipStream_t s, int taps = kTapNone, const float* zero = nullptr)
{
    const bool geglu = geglu_h > 0, skinny = form == LinForm::Skinny;
    const int tile = form == LinForm::Tile128 ? 128 : 64;   // rows per workgroup (skinny: 64 as well)
    if (nprob < 1 || nprob > kMaxProb || KS < 1 || K < KS || K > (1 << 20) || M % tile || (geglu && KS != 1)) return hipErrorInvalidValue;
    const int Kc = K / KS;
    if ((unsigned)taps > kTap3d) return hipErrorInvalidValue;
    // column tiles in grid.x: 16 (GEGLU: a value and a gate tile, 32) skinny; `tile` (GEGLU: 64 value + 64 gate columns)
    int tiles = 0;
    auto problems = [&](LinProb* p) {
        for (int i = 0; i < kMaxProb; ++i) {
            const LinSpec& sp = specs[i < nprob ? i : 0];
            p[i] = LinProb{sp.X, sp.W, sp.P, sp.bias, sp.N, tiles};
            if (i < nprob) tiles += skinny ? sp.N / (geglu ? 32 : 16) : geglu ? geglu_h / 64 : sp.N / tile;
        }
    };
    if (skinny) {   // grid (n-tiles, KS, M / 64), 512 threads
        LinArgs a;
        problems(a.p);
        a.nprob = nprob; a.M = M; a.Kc = Kc; a.ldx = ldx; a.ldw = ldw; a.geglu_h = geglu_h;
#ifdef AHV_ENC_PROBE
        a.stamps = AHV_ENC_STAMP_PTR;
#endif
        const dim3 grid(tiles, KS, M / 64);
        switch (lin_key(Kc, geglu, taps)) {
        case lin_key(256, false, kTapNone): AHV_ENC_LAUNCH((linear_staged_kernel<1, 256, false>), grid, dim3(512), 0, s, a); break;
        case lin_key(512, false, kTapNone): AHV_ENC_LAUNCH((linear_staged_kernel<1, 512, false>), grid, dim3(512), 0, s, a); break;
        case lin_key(512, true, kTapNone): AHV_ENC_LAUNCH((linear_staged_kernel<2, 512, true>), grid, dim3(512), 0, s, a); break;
        case lin_key(256, false, kTap2d): AHV_ENC_LAUNCH((linear_staged_kernel<1, 256, false, 1>), grid, dim3(512), 0, s, a); break;  // a tap per slice
        case lin_key(256, false, kTap3d): AHV_ENC_LAUNCH((linear_kernel<32>), grid, dim3(512), 0, s, a); break;  // 8 waves x 32 channels
        case lin_key(128, false, kTap3d): AHV_ENC_LAUNCH((linear_kernel<16>), grid, dim3(512), 0, s, a); break;  // 8 waves x 16 channels
        default: return hipErrorInvalidValue;
        }
    } else {        // grid (column tiles, M / tile, KS), 256 threads
        if ((Kc & 31) || (geglu_h & 63)) return hipErrorInvalidValue;   // an even number of 16-wide k-steps
        for (int i = 0; i < nprob; ++i)
            if (!geglu && specs[i].N % tile) return hipErrorInvalidValue;
        TileArgs a;
        problems(a.p);
        a.nprob = nprob; a.M = M; a.K = Kc; a.ldx = ldx; a.ldw = ldw; a.geglu_h = geglu_h; a.zero = zero;
#ifdef AHV_ENC_PROBE
        a.stamps = AHV_ENC_STAMP_PTR;
#endif
        const dim3 grid(tiles, M / tile, geglu ? 1 : KS);
        switch (lin_key(tile, geglu, taps)) {
        case lin_key(128, true, kTapNone): AHV_ENC_LAUNCH((linear_tile_kernel<true, 4>), grid, dim3(256), 0, s, a); break;
        case lin_key(128, false, kTapNone): AHV_ENC_LAUNCH((linear_tile_kernel<false, 4>), grid, dim3(256), 0, s, a); break;
        case lin_key(64, false, kTapNone): AHV_ENC_LAUNCH((linear_tile_kernel<false, 2>), grid, dim3(256), 0, s, a); break;
        case lin_key(64, false, kTap2d):   // the 3 x 3 convolution as an implicit GEMM (K = 9 x 256)
            if (K != 2304 || ldx != 256 || zero == nullptr) return hipErrorInvalidValue;
            AHV_ENC_LAUNCH((linear_tile_kernel<false, 2, true>), grid, dim3(256), 0, s, a);
            break;
        default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

size_t transformer_workspace_floats(int B) { return plan_transformer_workspace_floats(B); }

struct StreamWs {
    float *qkv, *kv, *att, *cat, *part, *tmp;
};

static StreamWs carve(float* ws, size_t M, int which)
{
    typedef BlockRowFloats L;
    float* b = ws + (size_t)which * M * L::total;
    StreamWs w;
    w.qkv = b;                b += M * L::qkv;
    w.kv = b;                 b += M * L::kv;
    w.att = b;                b += M * L::att;
    w.cat = b;                b += M * L::cat;
    w.part = b;               b += M * L::part;
    w.tmp = b;
    return w;
}

// One BasicTransformerBlock on EACH stream in the same launches: stream s uses weights w[s], input x[s],
// attention context ctx[s] (== x[s] for self-attention) and writes out[s].
static int run_block_pair(const EncPlan& plan, const ahv_block_weights* const w[2], const float* const x[2],
                          const float* const ctx[2], bool self_attn, float* const out[2], const StreamWs ws[2], hipStream_t s,
                          const char** what)
{
    const int M = plan.M, B = M / 64;
    const LinForm f256 = plan.tile64 ? LinForm::Tile64 : LinForm::Skinny;
    const LinForm ff = plan.ff_tiled ? LinForm::Tile128 : LinForm::Skinny;
    hipError_t e;
#define AHV_TRY(call, name) do { e = (call); if (e != hipSuccess) { *what = name; return (int)e; } } while (0)
    AttnOutArgs ao;  // q, k, v of each stream (row strides ldq / ldkv), W_out, one output slab per head in `part`
    ao.B = B;
    ao.scale = 0.125f;  // dim_head ** -0.5
    if (self_attn) {
        LinSpec sp[2];
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{x[i], w[i]->w_qkv, ws[i].qkv, nullptr, 768};
        AHV_TRY(launch_linear(f256, sp, 2, 256, 256, M, 256, 1, 0, s), "qkv projection");
        for (int i = 0; i < 2; ++i)
            ao.p[i] = AttnOutProb{ws[i].qkv, ws[i].qkv + 256, ws[i].qkv + 512, w[i]->w_out, ws[i].part, 768, 768};
    } else {
        LinSpec sq[2], skv[2];
        for (int i = 0; i < 2; ++i) {
            sq[i] = LinSpec{x[i], w[i]->w_qkv, ws[i].qkv, nullptr, 256};
            skv[i] = LinSpec{ctx[i], w[i]->w_qkv + 256 * 256, ws[i].kv, nullptr, 512};
        }
        LinSpec sp[4] = {sq[0], sq[1], skv[0], skv[1]};
        AHV_TRY(launch_linear(f256, sp, 4, 256, 256, M, 256, 1, 0, s), "q / kv projections");
        for (int i = 0; i < 2; ++i)
            ao.p[i] = AttnOutProb{ws[i].qkv, ws[i].kv, ws[i].kv + 256, w[i]->w_out, ws[i].part, 256, 512};
    }
    {   // attention and the output projection in ONE launch, then norm1 + concat
#ifdef AHV_ENC_PROBE
        ao.stamps = AHV_ENC_STAMP_PTR;
#endif
        if (plan.attn_per_pair) AHV_ENC_LAUNCH(attention_sample_head_kernel, dim3(2 * B, 4), dim3(256), 0, s, ao, M);
        else AHV_ENC_LAUNCH(attention_heads_kernel, dim3(2 * B, 4, 4), dim3(256), 0, s, ao, M);
        AHV_TRY(hipGetLastError(), "attention + out projection");
        LnArgs ln;
        ln.KS = 4; ln.M = M;  // one slab per head
        for (int i = 0; i < 2; ++i) ln.p[i] = LnProb{ws[i].part, w[i]->b_out, w[i]->ln1_g, w[i]->ln1_b, x[i], ws[i].cat};
        AHV_ENC_LAUNCH((ln_kernel<true, 4>), dim3((M + 3) / 4, 2), dim3(256), 0, s, ln);
        AHV_TRY(hipGetLastError(), "norm1 + concat");
    }
    {
        LinSpec sp[2];
        // FF in + GEGLU: writes the gated activations [M][2048] into `part`
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{ws[i].cat, w[i]->w_ff1, ws[i].part, w[i]->b_ff1, 4096};
        AHV_TRY(launch_linear(ff, sp, 2, 512, 512, M, 512, 1, 2048, s), plan.ff_tiled ? "ff in + geglu (tiled)" : "ff in + geglu");
        // FF out: ff_out_ks slabs [M][256] per stream, then norm2 + residual over them
        float* slab[2];
        for (int i = 0; i < 2; ++i) {
            slab[i] = plan.ff_out_in_part ? ws[i].part + (size_t)M * 2048 : ws[i].qkv;
            sp[i] = LinSpec{ws[i].part, w[i]->w_ff2, slab[i], nullptr, 256};
        }
        AHV_TRY(launch_linear(ff, sp, 2, 2048, 2048, M, 2048, plan.ff_out_ks, 0, s),
                plan.ff_tiled ? (plan.ff_out_ks == 8 ? "ff out (tiled, split-K 8)" : "ff out (tiled, split-K 4)")
                              : (plan.ff_out_ks == 8 ? "ff out (split-K 8)" : "ff out"));
        LnArgs ln;
        ln.KS = plan.ff_out_ks; ln.M = M;
        for (int i = 0; i < 2; ++i) ln.p[i] = LnProb{slab[i], w[i]->b_ff2, w[i]->ln2_g, w[i]->ln2_b, x[i], out[i]};
        if (plan.ff_out_ks == 8) AHV_ENC_LAUNCH((ln_kernel<false, 8>), dim3((M + 3) / 4, 2), dim3(256), 0, s, ln);
        else AHV_ENC_LAUNCH((ln_kernel<false, 4>), dim3((M + 3) / 4, 2), dim3(256), 0, s, ln);
        AHV_TRY(hipGetLastError(), "norm2 + residual");
    }
#undef AHV_TRY
    return 0;
}

int transformer_blocks(const ahv_block_weights* blocks, int depth, float* x_src, float* x_tgt, int B, float* ws,
                       hipStream_t s, const char** what)
{
    const EncPlan plan = plan_encoder(B);
    const StreamWs w2[2] = {carve(ws, plan.M, 0), carve(ws, plan.M, 1)};
    for (int d = 0; d < depth; ++d) {
        const ahv_block_weights* w = blocks + 4 * d;  // order: attn_self_1, attn_self_2, attn_cross_1, attn_cross_2
        int rc;
        {   // x = self_1(x); ctx = self_2(ctx)
            const ahv_block_weights* const ww[2] = {w + 0, w + 1};
            const float* const xin[2] = {x_src, x_tgt};
            float* const out[2] = {w2[0].tmp, w2[1].tmp};
            if ((rc = run_block_pair(plan, ww, xin, xin, true, out, w2, s, what))) return rc;
        }
        {   // x_out = cross_1(x, ctx); ctx_out = cross_2(ctx, x): both read the post-self tensors
            const ahv_block_weights* const ww[2] = {w + 2, w + 3};
            const float* const xin[2] = {w2[0].tmp, w2[1].tmp};
            const float* const cin[2] = {w2[1].tmp, w2[0].tmp};
            float* const out[2] = {x_src, x_tgt};
            if ((rc = run_block_pair(plan, ww, xin, cin, false, out, w2, s, what))) return rc;
        }
    }
    return 0;
}

// ---- whole forward_2d3d (modules/modules.py:86-101, inference form) --------------------------------------
// Activations live token-major [M = 64*B][C] ("channel-last").
size_t forward_2d3d_workspace_floats(int B) { return plan_forward_2d3d_workspace_floats(B); }

struct EncWs {
    float *T0, *S, *E0, *H1, *Xin, *Gn, *Xs, *Vol0, *H3, *Skip;
};

static EncWs carve_enc(float* ws, size_t M, int which)
{
    typedef EncRowFloats L;
    float* b = ws + (size_t)which * M * L::total;
    EncWs w;
    w.T0 = b;                 b += M * L::T0;
    w.S = b;                  b += M * L::S;
    w.E0 = b;                 b += M * L::E0;
    w.H1 = b;                 b += M * L::H1;
    w.Xin = b;                b += M * L::Xin;
    w.Gn = b;                 b += M * L::Gn;
    w.Xs = b;                 b += M * L::Xs;
    w.Vol0 = b;               b += M * L::Vol0;
    w.H3 = b;                 b += M * L::H3;
    w.Skip = b;
    return w;
}

static hipError_t launch_finish(const float* const P[2], const float* const bias[2], const float* const res[2],
                                float* const out[2], const float* pe, int KS, int M, int N, int ldp, int col0,
                                int relu_cols, int ldres, int ldo, int layout, hipStream_t s,
                                float* const out2[2] = nullptr)
{
    FinArgs a;
    for (int i = 0; i < 2; ++i)
        a.p[i] = FinProb{P[i], bias ? bias[i] : nullptr, res ? res[i] : nullptr, out[i], out2 ? out2[i] : nullptr};
    a.pe = pe; a.KS = KS; a.M = M; a.N = N; a.ldp = ldp; a.col0 = col0;
    a.relu_cols = relu_cols; a.ldres = ldres; a.ldo = ldo; a.layout = layout;
    const long n = (long)M * (N / 4);
    const dim3 grid((unsigned)((n + 255) / 256), 2);
    if (KS == 1) AHV_ENC_LAUNCH(finish_kernel<1>, grid, dim3(256), 0, s, a);
    else if (KS == 2) AHV_ENC_LAUNCH(finish_kernel<2>, grid, dim3(256), 0, s, a);
    else if (KS == 3) AHV_ENC_LAUNCH(finish_kernel<3>, grid, dim3(256), 0, s, a);
    else if (KS == 4) AHV_ENC_LAUNCH(finish_kernel<4>, grid, dim3(256), 0, s, a);
    else if (KS == 9) AHV_ENC_LAUNCH(finish_kernel<9>, grid, dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

int forward_2d3d(const ahv_aligner_weights* w, const float* l4_src, const float* l4_tgt, int B, float* ws,
                 float* vol_src, float* vol_tgt, hipStream_t s, const char** what)
{
    const EncPlan plan = plan_encoder(B);
    const int M = plan.M, MV = 512 * B;
    const LinForm f256 = plan.tile64 ? LinForm::Tile64 : LinForm::Skinny;
    const LinForm fconv = plan.conv_tiled ? LinForm::Tile64 : LinForm::Skinny;
    const EncWs e[2] = {carve_enc(ws, M, 0), carve_enc(ws, M, 1)};
    float* tws = ws + 2 * (size_t)M * EncRowFloats::total;
    float* zero_row = ws + forward_2d3d_workspace_floats(B) - kEncZeroRowFloats;
    hipError_t err;
#define AHV_TRY(call, name) do { err = (call); if (err != hipSuccess) { *what = name; return (int)err; } } while (0)
#define PAIR(T, name, a0, a1) T const name[2] = {a0, a1}
    {   // (B,768,8,8) -> tokens [M][768]
        Nchw2TokArgs a;
        a.in[0] = l4_src; a.in[1] = l4_tgt; a.out[0] = e[0].T0; a.out[1] = e[1].T0; a.C = 768; a.B = B;
        a.zero = zero_row;
        AHV_ENC_LAUNCH(nchw_to_tokens_kernel, dim3(768 / 64, B, 2), dim3(256), 0, s, a);
        AHV_TRY(hipGetLastError(), "layout");
    }
    PAIR(const float*, S, e[0].S, e[1].S);
    PAIR(float*, E0, e[0].E0, e[1].E0);
    PAIR(float*, H1, e[0].H1, e[1].H1);
    PAIR(float*, Xin, e[0].Xin, e[1].Xin);
    PAIR(float*, Vol0, e[0].Vol0, e[1].Vol0);
    PAIR(float*, H3, e[0].H3, e[1].H3);
    PAIR(float*, Skip, e[0].Skip, e[1].Skip);
    {   // feature_embedding: conv1x1 768->256, then res-block (conv3x3, relu, conv3x3, + skip), then + pos-emb
        LinSpec sp[2];
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{e[i].T0, w->w_emb, e[i].S, nullptr, 256};
        AHV_TRY(launch_linear(LinForm::Skinny, sp, 2, 768, 768, M, 768, 3, 0, s), "embedding conv1x1");
        AHV_TRY(launch_finish(S, nullptr, nullptr, E0, nullptr, 3, M, 256, 256, 0, 0, 0, 256, 0, s), "embedding sum");
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{e[i].E0, w->w_conv1, e[i].S, nullptr, 256};
        const int cks = plan.conv_ks;
        AHV_TRY(launch_linear(fconv, sp, 2, 256, 2304, M, 2304, cks, 0, s, kTap2d, zero_row), plan.conv_tiled ? "res-block conv1 (tiles)" : "res-block conv1");
        AHV_TRY(launch_finish(S, nullptr, nullptr, H1, nullptr, cks, M, 256, 256, 0, 256, 0, 256, 0, s), "res-block relu");
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{e[i].H1, w->w_conv2, e[i].S, nullptr, 256};
        AHV_TRY(launch_linear(fconv, sp, 2, 256, 2304, M, 2304, cks, 0, s, kTap2d, zero_row), plan.conv_tiled ? "res-block conv2 (tiles)" : "res-block conv2");
        PAIR(const float*, resE0, e[0].E0, e[1].E0);
        AHV_TRY(launch_finish(S, nullptr, resE0, Xin, w->posemb, cks, M, 256, 256, 0, 0, 256, 256, 0, s), "res-block skip + posemb");
    }
    {   // BidirectionTransformer: shared GroupNorm, per-stream proj_in, blocks, per-stream proj_out + residual
        GnArgs g;
        g.x[0] = e[0].Xin; g.x[1] = e[1].Xin; g.y[0] = e[0].Gn; g.y[1] = e[1].Gn; g.g = w->gn_g; g.be = w->gn_b; g.B = B;
        AHV_ENC_LAUNCH(groupnorm_kernel, dim3(8, B, 2), dim3(256), 0, s, g);
        AHV_TRY(hipGetLastError(), "groupnorm");
        LinSpec sp[2];
        // proj_in with its bias added in the linear's epilogue (one K slice): straight into the token buffer
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{e[i].Gn, w->w_in[i], e[i].Xs, w->b_in[i], 256};
        AHV_TRY(launch_linear(f256, sp, 2, 256, 256, M, 256, 1, 0, s), "proj_in + bias");
        const int rc = transformer_blocks(w->blocks, w->depth, e[0].Xs, e[1].Xs, B, tws, s, what);
        if (rc) return rc;
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{e[i].Xs, w->w_out[i], e[i].S, nullptr, 256};
        AHV_TRY(launch_linear(f256, sp, 2, 256, 256, M, 256, 1, 0, s), "proj_out");
        PAIR(const float*, bout, w->b_out[0], w->b_out[1]);
        PAIR(const float*, resX, e[0].Xin, e[1].Xin);
        // + bias + x_in, written as the channel-last volume [B][8][8][8][32] (channel 256 = c' * 8 + d)
        AHV_TRY(launch_finish(S, bout, resX, Vol0, nullptr, 1, M, 256, 256, 0, 0, 256, 0, 1, s), "proj_out + residual");
    }
    {   // feature_embedding_3d: conv3d 32->16, relu, conv3d 16->16, + 1x1x1 skip (folded into conv1 as columns 16..31)
        LinSpec sp[2];
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{e[i].Vol0, w->w3d_1, e[i].S, nullptr, 32};
        AHV_TRY(launch_linear(LinForm::Skinny, sp, 2, 32, 1024, MV, 1024, 4, 0, s, kTap3d), "conv3d 1 + skip");
        // columns 0..15 = conv1 (ReLU) -> H3, columns 16..31 = the 1x1x1 skip -> Skip: one pass over the 4 slabs
        AHV_TRY(launch_finish(S, nullptr, nullptr, H3, nullptr, 4, MV, 32, 32, 0, 16, 0, 0, 3, s, Skip), "conv3d relu | skip");
        PAIR(float*, S2, e[0].S + (size_t)MV * 32 * 4, e[1].S + (size_t)MV * 32 * 4);
        for (int i = 0; i < 2; ++i) sp[i] = LinSpec{e[i].H3, w->w3d_2, S2[i], nullptr, 16};
        AHV_TRY(launch_linear(LinForm::Skinny, sp, 2, 16, 512, MV, 512, 4, 0, s, kTap3d), "conv3d 2");
        PAIR(const float*, S2c, S2[0], S2[1]);
        PAIR(const float*, resS, e[0].Skip, e[1].Skip);
        PAIR(float*, vout, vol_src, vol_tgt);
        AHV_TRY(launch_finish(S2c, nullptr, resS, vout, nullptr, 4, MV, 16, 16, 0, 0, 16, 0, 2, s), "volume");
    }
#undef PAIR
#undef AHV_TRY
    return 0;
}

}  // namespace ahv
