// The one-launch layer of a REAL-valued adjacency (graphs of <= 32 nodes) under the gates' training-mode dropout:
// ggcn_layer_fused_weighted_drop.  Argument checks and shape classes are launch_fused's (fused_layer.hip).
#include "fused_common.h"

namespace ggcn {
namespace {

// ggcn_layer_fused_weighted_drop: the layer of a REAL-valued adjacency (graphs of <= 32 nodes, ggcn_graph_operands_weighted blocks)
// under the gates' training-mode dropout (bert_amir5.py:621-625) -- layer_fused_kernel's float32 path for ONE part that always
// ends in the MID epilogue with the DROP element math (fused_common.h: out = v*sg*k_store, the pools maximise v*g*k element by
// element).  A kernel of its own, chosen by the launcher: a run-time branch to this epilogue inside layer_fused_kernel moves the
// registers of the forms that exist (measured: 8 of its 28 instantiations, +2 VGPRs on the headline class, 12 -> 24 bytes of
// scratch on the general f16mx8 form).  The epilogue's operands take the register staging (the keep factors' launch never had
// the LDS-DMA form); no overlap operands, no second part, no stamps.
// A file of its own as well: instantiated inside fused_layer.hip, these kernels moved the register allocation of two of that
// file's general f16mx8 forms (251 -> 245 and 256 -> 253 VGPRs), and every kernel that exists keeps its resource report.
// The prologue and the main-loop call below are therefore a COPY of layer_fused_kernel's, on purpose: do not fold the two into a
// shared helper without comparing `make resources` of fused_layer.hip before and after -- code shared with that file is what moved
// its registers.  A change to the staging or the main-loop call there has to be made here as well.
// Shape classes: T = 32 with B % 4 == 0 but WITHOUT vector stores has no unguarded (FULLT) instantiation here and runs the guarded
// form -- same results, a few compares per row (launch_fused_weighted_drop below has the reason).
template <int SCH, bool AVEC, bool KFULL, bool FULLT, bool VST>
__global__ __launch_bounds__(kThreads, kWavesPerSimd) void layer_fused_weighted_drop_kernel(const FusedArgs a)
{
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes + kEpiLdsBytes + GGCN_LAB_LDS_PAD];
    const int B = a.B, T = a.T, K = a.K, F = a.F;
    int g_tile, n_wgi;
    if (!tile_of_block(blockIdx.x, a.g_tiles, a.n_wg, g_tile, n_wgi)) return;
    const LayerPart &lp = a.part[0];
    const char *__restrict__ wpack = lp.wpack;

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int gt0 = g_tile * (4 * WM);  // graph slots of 32 rows in this workgroup's tile
    const int g0 = gt0 + wm * 4;        // this wavefront's 4 graphs
    const int n_tiles_total = (F + NT - 1) / NT;
    const int nt0 = n_wgi * (BN / NT) + wn * RN;

    // tile row 32*slot + r  <->  node r of graph g0+slot
    constexpr int NP = Geom<float>::NP;
    const float *arow[NP];
    bool avalid[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int row = stage_row<float>(i);
        const int g = gt0 + (row >> 5), r = row & 31;
        avalid[i] = (g < B) && (FULLT || r < T);
        const int64_t node = avalid[i] ? (int64_t)g * T + r : 0;  // clamped, zeroed by the select
        arow[i] = a.X + node * a.ldx;
    }
    stage_epilogue_operands<kLdsBytes>(a, lp, g0, n_wgi, lds, tid);   // g0 = gt0: one wavefront row
    f32x16 acc[4][RN];
    if constexpr (SCH == 0)
        bx3::mainloop<float, AVEC, KFULL, !FULLT>(arow, avalid, wpack, K, a.k_steps, wm, nt0, n_tiles_total, lds, acc);
    else {
        float amax;
        constexpr bool BUF = AVEC && KFULL;   // buffer loads, as in layer_fused_kernel
        mx8::BufX<float> bx;
        if constexpr (BUF) {
            int rel[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int row = stage_row<float>(i);
                rel[i] = avalid[i] ? (row >> 5) * T + (row & 31) : -1;   // padding rows: outside the descriptor, zeros
            }
            bx = mx8::make_bufx<float>(a.X, a.ldx, (int64_t)gt0 * T, (int64_t)B * T, rel, tid);
        }
        mx8::mainloop<float, AVEC, KFULL, !FULLT, false, BUF>(arow, avalid, wpack, K, a.k_steps / 2, wm, nt0, n_tiles_total, lds, acc, 0, 4,
                                                             &amax, &bx);
        fused_range_verdict<kLdsBytes>(amax, wpack, (int64_t)n_tiles_total * (a.k_steps / 2) * mx8::STAGE_PACK_BYTES, lds, true);
    }
    if (lp.out) epilogue<SCH, FULLT, VST, true, true, kLdsBytes, true>(a, lp, acc, g0, nt0, n_tiles_total, lds, tid);
    else epilogue<SCH, FULLT, VST, true, false, kLdsBytes, true>(a, lp, acc, g0, nt0, n_tiles_total, lds, tid);
}

}  // namespace

// the shape classes of launch_fused's GGCN_PICK.  (T = 32 and B % 4 == 0 WITHOUT vector stores -- F % 4 != 0, a misaligned or an
// absent `out` -- takes the guarded form: its unguarded instantiation wanted 256 VGPRs + 20 bytes of scratch per lane in both
// main loops, and no kernel of this file may spill; the guards cost that rare class a few compares per row.)
int launch_fused_weighted_drop(const char *who, const FusedArgs &a, int precision, bool avec, bool kfull, bool fullt, bool vst, int64_t grid,
                               hipStream_t st)
{
#define GGCN_LAUNCH_WD(SC, AV, KF, FT, VS) \
    hipLaunchKernelGGL((layer_fused_weighted_drop_kernel<SC, AV, KF, FT, VS>), dim3((unsigned)grid), dim3(kThreads), 0, st, a)
#define GGCN_PICK_WD(SC)                                                                 \
    do {                                                                                 \
        if (avec && kfull && fullt && vst) GGCN_LAUNCH_WD(SC, true, true, true, true);   \
        else if (avec && kfull && vst) GGCN_LAUNCH_WD(SC, true, true, false, true);      \
        else if (avec && kfull) GGCN_LAUNCH_WD(SC, true, true, false, false);            \
        else if (avec) GGCN_LAUNCH_WD(SC, true, false, false, false);                    \
        else GGCN_LAUNCH_WD(SC, false, false, false, false);                             \
    } while (0)
    if (precision == GGCN_PREC_F16MX8) GGCN_PICK_WD(1);
    else GGCN_PICK_WD(0);
#undef GGCN_PICK_WD
#undef GGCN_LAUNCH_WD
    return check_launch(who);
}

GGCN_RANGE_FLAG_TU(range_flag_weighted_drop)

}  // namespace ggcn
