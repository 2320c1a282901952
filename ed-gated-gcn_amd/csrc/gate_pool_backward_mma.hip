// Backward of the gate / max-pool epilogue AND the transposed aggregation in one launch, on the matrix cores (graphs of <= 32
// nodes, 0/1 adjacency, no gate dropout):
//
//   dY[t] = d_out[t]*sg + [t = argmax_a] d_pa*ga + [t = argmax_b] d_pb*gb         models/bert_amir5.py:627-640 backwards
//   dH    = A^T . D . dY,   D = diag(1 / (rowsum(A) + 1))                           models/gcn.py:35,41 backwards (train.py:120)
//
// gate_pool_backward_agg_kernel (gate_pool_backward.hip) keeps 32 x 4 sums per thread and scatters every dY row into the rows
// its mask names: 1024 scalar bit tests per thread, 431 us per layer at config 2 -- the largest kernel of the training step.
// Here dH_g [32 x F] = (A_g^T) [32 x 32] . (D.dY_g) [32 x F] is what it looks like: one MFMA chain per (graph, 32 columns), as
// in the forward's epilogue (fused_common.h).  The tile -- the lane -> row map, the buffer-resource loads, the pools' winners, dY,
// the three-plane split, the gate gradients' store, dH through LDS -- is gate_pool_backward_tile.h, shared with the three other
// one-launch forms.  This file's own:
//   * ONE workgroup per graph, streamed once: a first form with a workgroup per (graph, 256 columns) spread a graph's 3 KiB rows
//     over three XCDs and ran 612 us where this one runs 292.  Its four wavefronts walk the 64-column groups w, w + 4, ...; a
//     group = two 32-column tiles, one pass each: all of a graph's rows are one 32-row block;
//   * dY x 1/(deg + 1) in three bf16 planes (residual 2^-25: gradients have no range contract, and the parity test wants dH to a
//     few fp32 ulps of its scale) times A^T, an exact 0/1 operand held in registers: 6 MFMAs per tile;
//   * A^T's fragments come from ggcn_graph_operands blocks of the TRANSPOSED row masks (ggcn_rowmask_transpose, once per
//     adjacency tensor), 1/(deg + 1) in register order from the graph's own blocks -- nothing about a graph is computed here;
//   * max |dH| (ggcn_linear_scaled's scale) falls out of the accumulators.
// Traffic: out + d_out read once (the scalar kernel reads d_out twice), dH written once: 1.2 GB in 292 us at config 2 (4.1 TB/s;
// the scalar form on the same box: 395-400 us).  149 VGPRs, no scratch, 32 KiB of LDS: three workgroups per CU.
// pa_g / pb_g are formed right before the loop over the rows on purpose: see dy_row in the tile header.
#include "gate_pool_backward_tile.h"

namespace ggcn {
namespace {

using namespace bx3;
using namespace gpb;

constexpr int kOpsBytesB = GGCN_GRAPH_OPS_BYTES;   // [0,1024) A fragments k-step 0, [1024,2048) k-step 1, [2048,2176) 1/(deg+1) float[h][16]

__global__ __launch_bounds__(256, 3) void gate_pool_backward_mma_kernel(
    const float *__restrict__ out, int64_t ldo, const float *__restrict__ store_gate, const float *__restrict__ gate_a,
    const float *__restrict__ gate_b, const float *__restrict__ d_out, int64_t ldd, const float *__restrict__ d_pa,
    const float *__restrict__ d_pb, const char *__restrict__ ops, const char *__restrict__ ops_t, int T, int F,
    float *__restrict__ dH, int64_t ldh, float *__restrict__ d_sg, float *__restrict__ d_ga, float *__restrict__ d_gb,
    float *__restrict__ d_bsum, unsigned int *__restrict__ dh_amax)
{
    __shared__ __attribute__((aligned(16))) float stage_all[4][32 * 64];   // per wavefront: 32 rows x 64 columns on their way to 16-byte stores
    const int b = blockIdx.x;          // one workgroup per graph: its rows are ONE contiguous block of `out` / `d_out` / dH
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    float *stage = stage_all[wave];

    // the graph's operands: A^T as the aggregation MFMA's A fragments (0xFFFF elements -> bf16 1.0), 1/(deg + 1) in register order
    bf16x8 aft[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(ops_t + (int64_t)b * kOpsBytesB + s * 1024 + lane * 16);
        union { bf16x8 v; uint32_t w[4]; } u;
        u.w[0] = raw.x & 0x3F803F80u; u.w[1] = raw.y & 0x3F803F80u; u.w[2] = raw.z & 0x3F803F80u; u.w[3] = raw.w & 0x3F803F80u;
        aft[s] = u.v;
    }
    float rinv[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 t = *reinterpret_cast<const float4 *>(ops + (int64_t)b * kOpsBytesB + 2048 + h * 64 + q * 16);
        rinv[4 * q] = t.x; rinv[4 * q + 1] = t.y; rinv[4 * q + 2] = t.z; rinv[4 * q + 3] = t.w;
    }

    float amax = 0.0f;
#pragma unroll 1
    for (int col0 = wave * 64; col0 < F; col0 += 256) {   // wavefront-uniform walk over this wavefront's 64-column groups
#pragma unroll 1   // (one tile at a time: ~100 registers instead of 175 -- four wavefronts per SIMD keep more loads in flight than two)
    for (int j = 0; j < 2; ++j) {
        if (col0 + 32 * j >= F) break;   // wavefront-uniform: the group's last tile
        const Column k = column_operands(b, col0 + 32 * j + c, F, store_gate, gate_a, gate_b, d_pa, d_pb);
        float ov[16], dv[16];
        GraphRows(out, ldo, d_out, ldd, b, T, F, h, k.colc).load(0, ov, dv);
        Winners w;
        scan_rows(w, k, ov, dv, 0, h, T);
        exchange_halves(w);
        // dY and D.dY in register order
        float gw[16], bsum = 0.0f;
        const float pa_g = k.dpa * k.ga, pb_g = k.dpb * k.gb;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float g = dy_row(k, w, dv[r], row_of(r, h), T, pa_g, pb_g);
            bsum += g;
            gw[r] = g * rinv[r];                                   // gcn.py:35: the row's own 1 / (deg + 1)
        }
        bsum += __shfl_xor(bsum, 32);
        w.acc_sg += __shfl_xor(w.acc_sg, 32);
        // dH tile = A^T . (D.dY)
        bf16x8 pl[3][2];
        split3(gw, pl);
        f32x16 y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = 0.0f;
        y = mma_01(aft, pl, y);
#pragma unroll
        for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(y[r]));   // (plain C: an inline-asm reader of a fresh MFMA result is a hazard the compiler does not pad)
        stage64_put(stage, y, j, c, h);
        store_column_grads(k, w, h, bsum, d_bsum, d_sg, d_ga, d_gb);
    }
    stage64_store(stage, dH, ldh, b, T, F, col0, lane);
    }   // column groups
    if (dh_amax) {
        if (!(amax <= 3.0e38f)) amax = __builtin_inff();   // NaN / inf in the gradients: say so
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
        if (lane == 0) atomicMax(dh_amax, __float_as_uint(amax));
    }
}

// row masks of the transposed adjacency, graphs of <= 32 nodes: one wavefront per graph, lane t holds row t's word; bit t of
// the word of row s = bit s of the word of row t (32 ballots)
__global__ __launch_bounds__(256) void rowmask_transpose_kernel(const uint32_t *__restrict__ rowmask, int B, int T,
                                                                uint32_t *__restrict__ rowmask_t)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= B) return;   // wavefront-uniform
    const uint32_t m = lane < T ? rowmask[(int64_t)g * T + lane] : 0u;
    uint32_t mt = 0u;
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const unsigned long long bal = __ballot((m >> s) & 1u);
        if (lane == s) mt = (uint32_t)bal;
    }
    if (lane < T) rowmask_t[(int64_t)g * T + lane] = mt;
}

}  // namespace
}  // namespace ggcn

using namespace ggcn;

extern "C" {

int ggcn_rowmask_transpose(const uint32_t *rowmask, int B, int T, uint32_t *rowmask_t, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    if (!rowmask || !rowmask_t) return fail(GGCN_EINVAL, "ggcn_rowmask_transpose: null pointer");
    if (B <= 0 || T <= 0) return fail(GGCN_EINVAL, "ggcn_rowmask_transpose: B=%d T=%d must be positive", B, T);
    if (T > 32) return fail(GGCN_EUNSUPPORTED, "ggcn_rowmask_transpose: T=%d > 32 (one word per node)", T);
    hipLaunchKernelGGL(rowmask_transpose_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, rowmask, B, T, rowmask_t);
    return check_launch("ggcn_rowmask_transpose");
}

int ggcn_gate_pool_backward_mma(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops,
                                const void *graph_ops_t, int B, int T, int F, float *dH, int64_t ldh, float *d_sg, float *d_ga,
                                float *d_gb, float *d_bsum, float *dh_amax, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_gate_pool_backward_mma";
    if (!out || !dH || !graph_ops || !graph_ops_t) return fail(GGCN_EINVAL, "%s: null pointer", who);
    const EntryRules rules = {who, false, 1, "", 32, "", false,
                              "F % 4 == 0, ldh % 4 == 0 and 16-byte aligned dH / operand blocks; use ggcn_gate_pool_backward_agg or the two calls"};
    // (the 2 GiB rule of this entry: ldo and ldd, whether d_out is there or not, and not ldh)
    if (const int rc = backward_entry_checks(rules, B, T, F, {ldo, ldh, d_out ? ldd : F}, {ldo, ldd},
                                             F % 4 == 0 && ldh % 4 == 0 && aligned16(dH) && aligned16(graph_ops) && aligned16(graph_ops_t)))
        return rc;
    hipLaunchKernelGGL(gate_pool_backward_mma_kernel, dim3((unsigned)B), dim3(256), 0, st, out, ldo, store_gate, gate_a, gate_b,
                       d_out, ldd, d_pa, d_pb, static_cast<const char *>(graph_ops), static_cast<const char *>(graph_ops_t), T, F,
                       dH, ldh, d_sg, d_ga, d_gb, d_bsum, reinterpret_cast<unsigned int *>(dh_amax));
    return check_launch(who);
}

}  // extern "C"
