// The argument blocks of the one-launch layer and block kernels, and the host functions that take them.  Plain structs and
// prototypes, no device code: capi.hip fills a FusedArgs by field name and hands it to a launcher; fused_common.h includes this
// header for the kernels.
#pragma once
#include "common.h"
#include "dropout_hash.h"

namespace ggcn {

// what one group of column tiles ("part") computes: part 0 = the layer itself (or layer 1 of the block),
// part 1 = layer 2 of the block through W12
struct LayerPart {
    const char *wpack;          // ggcn_weight_pack image of this part's [K, F] matrix
    const float *bias;          // added after the (last) normalised aggregation, or NULL
    const float *mid;           // NULL: one aggregation.  Else: y = D.A.(D.A.h + mid) + bias
    const float *pre;           // NULL, or [F] added to `hidden` BEFORE the aggregation (graphs of 33..256 nodes): y = D.A.(h + 1.pre^T) + bias
    const float *store_gate;    // [B,F] or NULL (ones)
    const float *pool_gate_a;   // [B,F] or NULL (ones)
    const float *pool_gate_b;
    float *out;                 // [N, ldo] or NULL
    float *pool_a, *pool_b;     // [B,F] or NULL
    float *ov_partial;          // [B, ceil(F/64)] or NULL: sum_f pool_a*pool_b per graph and 64 columns
    int ldo;
};

struct FusedArgs {
    const float *X;
    int64_t ldx;
    const uint32_t *rowmask;    // graphs of 33..256 nodes (layer_fused_wide_kernel)
    const char *graph_ops;      // graphs of <= 32 nodes: ggcn_graph_operands blocks (layer_fused_kernel); 129..256: optional edge-list blocks;
                                // layer_fused_wide_kernel<.., WEIGHTED>: ggcn_graph_operands_weighted_wide blocks (rowmask NULL)
    const char *graph_ops2;     // the block's W12 tiles: ggcn_graph_operands2 blocks ((D.A)^2 in the launch's plane type)
    const float *ov_in;         // partials an EARLIER launch wrote: block 0 reduces them to *ov_out first
    float *ov_out;
    int B, T, K, F;
    int g_tiles, n_wg, n_parts, k_steps;
    LayerPart part[2];
    DropSpec drop;              // training-mode keep masks of the gates (thr = 0: none); one part only
    unsigned long long *stamps; // diagnostics only (ggcn_debug_block_fused_stamped): [workgroup][2] = d(s_memtime), d(s_memrealtime) around the main loop
    const __bf16 *Xb;           // bf16 features (ggcn_layer_fused_bf16[_drop]: graphs of <= 32 nodes, ggcn_layer_fused_bf16_wide: 33..256;
                                // one layer, bf16x3 image); X then only names readable memory (the weight image) for the
                                // discarded fallback reads of an absent gate / bias
};

// an [N, ldo] output leaves as 16-byte row stores (they address a graph's rows with 32-bit byte offsets from its first row)
inline bool vector_row_stores(const FusedArgs &a, const LayerPart &lp)
{
    return (a.F % 4 == 0) && (lp.ldo % 4 == 0) && aligned16(lp.out) && (int64_t)a.T * lp.ldo * 4 < ((int64_t)1 << 31);
}

// What every one-launch kernel asks of the shape and of each part before it may launch: positive sizes, ldx >= K, a 16-byte aligned
// weight image, an output, its leading dimension and 32-bit offsets.  vst: every [N, ldo] output of the launch takes 16-byte row stores.
int fused_part_checks(const char *who, const FusedArgs &a, bool &vst);   // fused_layer.hip

// The rest of the argument checks and the launch of one layer (n_parts = 1) or of a described block; fills g_tiles, n_wg, k_steps.
// (weighted_block: ggcn_block_fused_weighted -- both parts on hi / lo operand blocks, kernels of their own in fused_weighted_drop.hip)
int launch_fused(const char *who, FusedArgs &a, int precision, hipStream_t st, bool weighted_block = false);   // fused_layer.hip

// one layer on ggcn_graph_operands_weighted_wide blocks (a.graph_ops), graphs of 33..128 nodes
int launch_fused_weighted_wide(const char *who, FusedArgs &a, int precision, hipStream_t st);   // fused_wide.hip

// The two-layer block: the entry describes layer 1 in part[0] and layer 2 in part[1] (n_parts = 2, graph_ops / graph_ops2 as
// given; zero_mid of the real-valued kind in part[0].mid); the launcher refuses, collapses to the eval form and launches.
enum BlockKind { kBlockBinary, kBlockWeighted, kBlockBf16 };   // 0/1 adjacency, real-valued adjacency, bf16 features
int launch_block(const char *who, FusedArgs &a, BlockKind kind, int precision, hipStream_t st);   // fused_layer.hip

// the eight-wavefront form of the block on the same description (fused_block8.hip)
constexpr int kBlock8RowMajor = 1, kBlock8NoDma = 2, kBlock8SameSlots = 4, kBlock8Prio = 8;
bool block8_shape(int B, int T, int K, int F);
bool block8_takes(const FusedArgs &a);
int block_fused8(const char *who, FusedArgs &a, int flags, hipStream_t st);

}  // namespace ggcn
