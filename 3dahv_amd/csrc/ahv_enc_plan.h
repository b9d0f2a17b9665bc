// ahv_enc_plan.h -- every shape decision of the encoder's host side (ahv_encoder.hip) as pure functions of the batch size
// and the problem shape: which attention kernel, which linear form, which K split, where the split-K slabs go, and the two
// workspace layouts.  Plain C++17, no HIP include: tests/test_encoder_plan_cpu.py compiles it with the host compiler and
// holds every row of plan_encoder(1 .. 130) to a restatement of the conditions.
//
// The problem shape is fixed (aligner.py checks it before the C ABI is called): 64 tokens x 256 channels per sample and
// stream, 4 heads x 64, FF width 2048 (GEGLU projection 4096), embedding 768 -> 256, 3 x 3 convolutions K = 9 x 256.
// M = 64 B token rows per stream; every launch carries both streams.
//
//   launch                        form and split                                                      first B
//   q / k / v, proj_in, proj_out  staged | 64-tiles (M >= 2048)                                       32
//   attention + out projection    per (sample, head, key tile) | per (sample, head) (192 pairs)      24
//   FF in + GEGLU, FF out         staged | 128-tiles (M >= 1024 and M % 128 = 0)                      16, 18, 20, ...
//   FF out, K split               skinny: 8 (M <= 128) | 4;  tiled: 8 (M <= 1024) | 4               3;  18
//   3 x 3 convolutions            skinny, a tap per K slice | 64-tiles, K split 4096 / M, at least 1  16 (4), 17 (3), 22 (2), 33 (1)
#pragma once
#include <stddef.h>

namespace ahv {

// (sample, head) pairs from which attention_sample_head_kernel runs (tools/kbench_enc, both kernels alternating on one box,
// us per forward: B = 8 -- 64 pairs -- 751 with the tile-wise kernel / 784 with the pair-wise one; B = 16: 1 106 / 1 111;
// B = 24: 1 606 / 1 596; B = 32: 1 919 / 1 895)
constexpr int kAttnPairMinWgs = 192;
// 128 x 128 tiles for the two FF projections: a skinny workgroup owns 64 rows x 16 or 32 columns and re-reads its X rows once
// per column tile -- right for 64 .. 512 rows (weights are the traffic), 44 % of the matrix peak at 2048
constexpr int kTileMinM = 1024;
// 256-wide projections (K = 256, N = 256 / 512 / 768) at many rows: 64 x 64 tiles instead of the skinny kernel, whose
// workgroups re-read their 64 x 256 X tile once per 16 output columns.  Measured per forward (tools/kbench_enc, graph):
// B = 32: 2040 -> 2012 us (17.3 against 21.5 us per launch); B = 16: 1238 -> 1253; B = 8: 753 -> 761; B = 4: 490 -> 508.
constexpr int kTile64MinM = 2048;
// skinny FF out: 8 K-splits up to B = 2, so that the 4 MB of W_ff2 stream through 256 workgroups instead of 128 (-3.6 % per
// forward at B = 1, even at B = 2, slower from B = 4 on)
constexpr int kFfOutKs8MaxM = 128;
// FF out on tiles: N = 256 gives only 2 column tiles per stream, so the K split has to fill the chip -- 8 ways up to M = 1024
// (B = 16: 256 workgroups instead of 128; forward 1 213 -> 1 117 us), 4 ways from M = 2048 (B = 32: 256 workgroups; 8 ways
// measured 1.3 % SLOWER there: 16 k-steps per workgroup and an 8-slab LayerNorm)
constexpr int kFfOutTiledKs8MaxM = 1024;
// the two 3 x 3 convolutions on the tile kernel from B = 16 on, K split so that 512 workgroups fill the chip
constexpr int kConvTileMinM = 1024;
constexpr int kConvTileWgRows = 4096;   // rows at which the unsplit grid has its 512 workgroups
constexpr int kConvTaps = 9;            // the skinny form: one tap per K slice

// Linear forms.  Skinny: 64 rows x 16 (32: GEGLU) columns per workgroup, K split over grid.y (linear_staged_kernel; the 3-D
// taps: linear_kernel).  Tile64 / Tile128: linear_tile_kernel<., 2 / 4>.
enum class LinForm { Skinny, Tile64, Tile128 };

// K per split: an even number of 16-wide k-steps (the tile kernel's K loop is unrolled by two)
inline bool tile128_eligible(int M, int K, int N, int geglu_h)
{
    if (M < kTileMinM || (M & 127) || (K & 31)) return false;
    return geglu_h > 0 ? (geglu_h % 64 == 0 && N == 2 * geglu_h) : (N % 128 == 0);
}

// up to four plain problems of widths n[0 .. nprob)
inline bool tile64_eligible(const int* n, int nprob, int M, int K)
{
    if (M < kTile64MinM || (M & 63) || (K & 31) || nprob > 4) return false;
    for (int i = 0; i < nprob; ++i)
        if (n[i] & 63) return false;
    return true;
}

struct EncPlan {
    int M;                  // token rows per stream
    bool attn_per_pair;     // one workgroup per (sample, head); else per (sample, head, 16-query tile)
    bool tile64;            // the 256-wide linears (q / k / v, proj_in, proj_out) on 64 x 64 tiles
    bool ff_tiled;          // FF in + GEGLU and FF out on 128 x 128 tiles
    int ff_out_ks;          // K split of FF out: 4 or 8 (= slabs the second LayerNorm sums)
    bool ff_out_in_part;    // its slabs [ks][M][256]: behind the gated activations in `part` (2048 of its 4096 floats per
                            // row are free: room for 8), else in the qkv + kv scratch (1280 per row, free by then: room for 4)
    bool conv_tiled;        // the 3 x 3 convolutions as an implicit GEMM on 64 x 64 tiles
    int conv_ks;            // their K split = slabs the finish pass sums: 1 .. 4 tiled, 9 skinny
};

inline EncPlan plan_encoder(int B)
{
    EncPlan p;
    const int M = 64 * B;
    p.M = M;
    p.attn_per_pair = 2 * B * 4 >= kAttnPairMinWgs;   // two streams, four heads
    const int n256[3] = {768, 256, 512};              // qkv | q, proj_in, proj_out | kv
    p.tile64 = tile64_eligible(n256, 3, M, 256);
    p.ff_tiled = tile128_eligible(M, 512, 4096, 2048);   // FF in decides; FF out (N = 256) follows it
    p.ff_out_ks = (p.ff_tiled ? M <= kFfOutTiledKs8MaxM : M <= kFfOutKs8MaxM) ? 8 : 4;
    p.ff_out_in_part = p.ff_out_ks == 8;
    p.conv_tiled = M >= kConvTileMinM && (M & 63) == 0;
    p.conv_ks = p.conv_tiled ? (M >= kConvTileWgRows ? 1 : kConvTileWgRows / M) : kConvTaps;
    return p;
}

// ---- workspaces: per-row float counts, read by the size functions and by the carves ------------------------------------
// transformer blocks, per token row and stream
struct BlockRowFloats {
    static constexpr size_t qkv = 768;     // q | k | v (self) or q (cross); with kv the 4 FF-out slabs
    static constexpr size_t kv = 512;      // k | v of the other stream (cross)
    static constexpr size_t att = 256;     // spare
    static constexpr size_t cat = 512;     // [x, norm1(attention)]
    static constexpr size_t part = 4096;   // per-head slabs of attention + out projection; gated activations | 8 FF-out slabs
    static constexpr size_t tmp = 256;     // ping-pong tokens
    static constexpr size_t total = qkv + kv + att + cat + part + tmp;
};

// forward_2d3d around the blocks, per token row and stream
struct EncRowFloats {
    static constexpr size_t T0 = 768;      // tokens of layer 4
    static constexpr size_t S = 2304;      // split-K slabs of whichever linear runs
    static constexpr size_t E0 = 256, H1 = 256, Xin = 256, Gn = 256, Xs = 256, Vol0 = 256;
    static constexpr size_t H3 = 128, Skip = 128;   // 512 voxels x 16 channels per sample = 128 per token row
    static constexpr size_t total = T0 + S + E0 + H1 + Xin + Gn + Xs + Vol0 + H3 + Skip;
};

constexpr size_t kEncZeroRowFloats = 64;   // the workspace's last 256 bytes: the zero row of the implicit-GEMM convolutions

inline size_t enc_rows(int B) { return (size_t)64 * (size_t)(B > 0 ? B : 0); }

inline size_t plan_transformer_workspace_floats(int B) { return 2 * enc_rows(B) * BlockRowFloats::total + 64; }

inline size_t plan_forward_2d3d_workspace_floats(int B)
{
    return 2 * enc_rows(B) * EncRowFloats::total + plan_transformer_workspace_floats(B) + kEncZeroRowFloats;
}

}  // namespace ahv
