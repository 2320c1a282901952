// The opt-in launches on a REAL-valued adjacency (graphs of <= 32 nodes) that have kernels of their own:
//   ggcn_layer_fused_weighted_drop   the one-launch layer under the gates' training-mode dropout;
//   ggcn_block_fused_weighted        the two-layer inference block in one launch, and its builder ggcn_graph_operands2_weighted.
// Argument checks and shape classes are launch_fused's (fused_layer.hip).
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
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes + kEpiLdsBytes];
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

// ---- ggcn_block_fused_weighted: the inference block of a REAL-valued adjacency in one launch ------------------------------------
namespace {

// ggcn_graph_operands2_weighted: M2 = (D.A_w)^2 * 2^10 per graph as hi / lo A-operand fragments of the plane type and
// rowsum(D.A_w), in the format of ggcn_graph_operands2 (fused_common.h).  One wavefront per graph.  Lane (r, h) walks row r of the
// CSR as graph_operands_w_kernel does (edges in CSR order, as ggcn_aggregate sums them), keeps the 16 columns of
// M = D.A_w its fragments hold and leaves them in LDS (4 KiB per graph + padding); then
//   M2[r][c] = sum_j M[r][j] * M[j][c]     (fp32, j ascending over 0..T-1: a fixed order, no atomics)
// with row j's four columns per fragment group read as one 16-byte broadcast.  flag (optional): bit 0 when an entry of M2 * 2^10
// does not fit the plane type or is not finite (graph_operands_w_kernel's thresholds).
constexpr int kM2RowStride = 36;   // floats per row of M in LDS: 16-byte aligned rows, lanes of one column 4 banks apart
template <int PLANE>
__global__ __launch_bounds__(256) void graph_operands2_w_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                                const float *__restrict__ vals, int B, int T, char *__restrict__ ops2,
                                                                int *__restrict__ flag)
{
    __shared__ __attribute__((aligned(16))) float mlds[4][32 * kM2RowStride];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x * 4 + wv;
    const bool live = g < B;   // wavefront-uniform (every wavefront reaches the barrier)
    const int r = lane & 31, h = lane >> 5;
    const int64_t node0 = (int64_t)g * T;
    float a[16], wsum = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = 0.0f;
    if (live && r < T) {
        const int e1 = rowptr[node0 + r + 1];
        for (int e = rowptr[node0 + r]; e < e1; ++e) {
            const int c = colidx[e] - (int)node0;
            const float w = vals ? vals[e] : 1.0f;
            wsum += w;
            // column c sits in k-step c >> 4 as element 4 ((c >> 3) & 1) + (c & 3) of the lane half (c >> 2) & 1
            const int idx = ((unsigned)c < 32u && ((c >> 2) & 1) == h) ? (c >> 4) * 8 + ((c >> 3) & 1) * 4 + (c & 3) : -1;
#pragma unroll
            for (int q = 0; q < 16; ++q) a[q] += idx == q ? w : 0.0f;
        }
    }
    const float inv = 1.0f / (wsum + 1.0f);   // gcn.py:35
    float *m = mlds[wv];
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // elements 4q .. 4q + 3 = columns 16 (q >> 1) + 8 (q & 1) + 4h ..
        const int c0 = 16 * (q >> 1) + 8 * (q & 1) + 4 * h;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live && r < T) v = make_float4(a[4 * q] * inv, a[4 * q + 1] * inv, a[4 * q + 2] * inv, a[4 * q + 3] * inv);   // rows >= T: zeros
        *reinterpret_cast<float4 *>(m + r * kM2RowStride + c0) = v;
    }
    __syncthreads();
    if (!live) return;
    float a2[16], rsum = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) a2[e] = 0.0f;
    for (int j = 0; j < T; ++j) {
        const float mrj = m[r * kM2RowStride + j];
        rsum += mrj;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 mj = *reinterpret_cast<const float4 *>(m + j * kM2RowStride + 16 * (q >> 1) + 8 * (q & 1) + 4 * h);
            a2[4 * q] = fmaf(mrj, mj.x, a2[4 * q]);
            a2[4 * q + 1] = fmaf(mrj, mj.y, a2[4 * q + 1]);
            a2[4 * q + 2] = fmaf(mrj, mj.z, a2[4 * q + 2]);
            a2[4 * q + 3] = fmaf(mrj, mj.w, a2[4 * q + 3]);
        }
    }
    char *blk = ops2 + (int64_t)g * kOps2Bytes;
    bool bad = false;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        union { uint4 q; unsigned short u[8]; } hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = a2[8 * s + e] * kM2Scale;
            bad = bad || !(fabsf(v) < (PLANE == 1 ? 60000.0f : 3.0e38f));
            if constexpr (PLANE == 1) {
                const _Float16 vh = (_Float16)v, vl = (_Float16)(v - (float)vh);
                hi.u[e] = __builtin_bit_cast(unsigned short, vh);
                lo.u[e] = __builtin_bit_cast(unsigned short, vl);
            } else {
                const __bf16 vh = (__bf16)v, vl = (__bf16)(v - (float)vh);
                hi.u[e] = __builtin_bit_cast(unsigned short, vh);
                lo.u[e] = __builtin_bit_cast(unsigned short, vl);
            }
        }
        *reinterpret_cast<uint4 *>(blk + s * 1024 + lane * 16) = hi.q;
        *reinterpret_cast<uint4 *>(blk + 2048 + s * 1024 + lane * 16) = lo.q;
    }
    // rowsum(D.A_w) in accumulator order: lane idx (0..31) writes entry [h' = idx >> 4][r' = idx & 15]
    const int rr = lane & 15, hh = (lane >> 4) & 1;
    const int row = (rr & 3) + 8 * (rr >> 2) + 4 * hh;
    const float rs = __shfl(rsum, row);
    if (lane < 32) reinterpret_cast<float *>(blk + 4096)[lane] = rs;
    if (bad && flag) atomicOr(flag, 1);
}

// ggcn_block_fused_weighted: layer_fused_kernel's float32 path for the block (W1 tiles on four XCDs, W12 tiles on the other four;
// or the W12 tiles alone: the eval form) where BOTH parts end in the MID epilogue -- part 0 on M = D.A_w (ggcn_graph_operands_weighted
// blocks, a.graph_ops) with the zero `mid` row, part 1 on M2 = (D.A_w)^2 (ggcn_graph_operands2_weighted blocks, a.graph_ops2) with
// bias_mid -- so the two halves of the grid carry equal epilogue work.  The one difference to layer_fused_kernel is where the
// epilogue's operand blocks come from: `mid` cannot choose the array here, the kernel names it (stage_epilogue_operands<.., GIVEN>).
// Kernels of their own for the reason layer_fused_weighted_drop_kernel has above: ggcn_block_fused's instantiations keep their
// code.  The prologue and the main-loop call are a COPY of layer_fused_kernel's; a change there has to be made here as well.
template <int SCH, bool AVEC, bool KFULL, bool FULLT, bool VST>
__global__ __launch_bounds__(kThreads, kWavesPerSimd) void block_fused_weighted_kernel(const FusedArgs a)
{
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes + kEpiLdsBytes];
    const int B = a.B, T = a.T, K = a.K, F = a.F;
    int g_tile, n_wgi;
    bool second = false;
    if (a.n_parts == 1) {   // the eval form: every XCD runs W12 tiles
        if (!tile_of_block(blockIdx.x, a.g_tiles, a.n_wg, g_tile, n_wgi)) return;
    } else {                // the block ids that share an XCD work on the same part (layer_fused_kernel has the measurements)
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        second = xcd >= 4;
        g_tile = (slot / a.n_wg) * 4 + (xcd & 3);
        n_wgi = slot % a.n_wg;
        if (g_tile >= a.g_tiles) return;
    }
    const LayerPart &lp = a.part[second ? 1 : 0];
    const char *__restrict__ wpack = lp.wpack;
    // layer 1's tiles read M, layer 2's (the only part of the eval form) M2: same block format, arrays of their own
    const char *ops_src = (a.n_parts == 2 && !second) ? a.graph_ops : a.graph_ops2;

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
    // whole tiles with aligned rows: the epilogue's operands come by LDS-DMA (layer_fused_kernel's condition; `mid` is never NULL here)
    const bool dma_stage = SCH == 1 && (a.n_wg * BN == F) && (gt0 + 4 <= B) && (F % 4 == 0) &&
                           ((reinterpret_cast<uintptr_t>(lp.store_gate) | reinterpret_cast<uintptr_t>(lp.pool_gate_a) | reinterpret_cast<uintptr_t>(lp.pool_gate_b) |
                             reinterpret_cast<uintptr_t>(lp.bias) | reinterpret_cast<uintptr_t>(lp.mid)) & 15u) == 0;
    if (dma_stage) stage_epilogue_operands_dma<kLdsBytes, true>(a, lp, g0, n_wgi, lds, tid, ops_src);
    else stage_epilogue_operands<kLdsBytes, true>(a, lp, g0, n_wgi, lds, tid, ops_src);   // g0 = gt0: one wavefront row
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
        if (dma_stage) dma_range_verdict<kLdsBytes>(amax, wpack, (int64_t)n_tiles_total * (a.k_steps / 2) * mx8::STAGE_PACK_BYTES, lds, tid & 63);
        else fused_range_verdict<kLdsBytes>(amax, wpack, (int64_t)n_tiles_total * (a.k_steps / 2) * mx8::STAGE_PACK_BYTES, lds, true);
    }
    if (lp.out) epilogue<SCH, FULLT, VST, true, true>(a, lp, acc, g0, nt0, n_tiles_total, lds, tid);
    else epilogue<SCH, FULLT, VST, true, false>(a, lp, acc, g0, nt0, n_tiles_total, lds, tid);
}

}  // namespace

// the shape classes of launch_fused's GGCN_PICK, one for one
int launch_fused_block_weighted(const char *who, const FusedArgs &a, int precision, bool avec, bool kfull, bool fullt, bool vst, int64_t grid,
                                hipStream_t st)
{
#define GGCN_LAUNCH_WB(SC, AV, KF, FT, VS) \
    hipLaunchKernelGGL((block_fused_weighted_kernel<SC, AV, KF, FT, VS>), dim3((unsigned)grid), dim3(kThreads), 0, st, a)
#define GGCN_PICK_WB(SC)                                                                 \
    do {                                                                                 \
        if (avec && kfull && fullt && vst) GGCN_LAUNCH_WB(SC, true, true, true, true);   \
        else if (avec && kfull && fullt) GGCN_LAUNCH_WB(SC, true, true, true, false);    \
        else if (avec && kfull && vst) GGCN_LAUNCH_WB(SC, true, true, false, true);      \
        else if (avec && kfull) GGCN_LAUNCH_WB(SC, true, true, false, false);            \
        else if (avec) GGCN_LAUNCH_WB(SC, true, false, false, false);                    \
        else GGCN_LAUNCH_WB(SC, false, false, false, false);                             \
    } while (0)
    if (precision == GGCN_PREC_F16MX8) GGCN_PICK_WB(1);
    else GGCN_PICK_WB(0);
#undef GGCN_PICK_WB
#undef GGCN_LAUNCH_WB
    return check_launch(who);
}

GGCN_RANGE_FLAG_TU(range_flag_weighted_drop)

}  // namespace ggcn

using namespace ggcn;

extern "C" {

int ggcn_graph_operands2_weighted(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, int plane, void *ops2,
                                  int32_t *flag, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_graph_operands2_weighted";
    if (!rowptr || !colidx || !ops2) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (B <= 0 || T <= 0) return fail(GGCN_EINVAL, "%s: B=%d T=%d must be positive", who, B, T);
    if (T > 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 32 (the two-layer block takes graphs of <= 32 nodes)", who, T);
    if (plane != 0 && plane != 1) return fail(GGCN_EINVAL, "%s: plane %d (0 = bf16 pairs, 1 = fp16 pairs)", who, plane);
    if (!aligned16(ops2)) return fail(GGCN_EINVAL, "%s: the blocks must be 16-byte aligned", who);
    if ((int64_t)B * T >= (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: B*T does not fit int32 node ids", who);
    const dim3 grid((unsigned)((B + 3) / 4));
    if (plane == 1) hipLaunchKernelGGL(graph_operands2_w_kernel<1>, grid, dim3(256), 0, st, rowptr, colidx, vals, B, T, static_cast<char *>(ops2), flag);
    else hipLaunchKernelGGL(graph_operands2_w_kernel<0>, grid, dim3(256), 0, st, rowptr, colidx, vals, B, T, static_cast<char *>(ops2), flag);
    return check_launch(who);
}

}  // extern "C"
