// Backward of the gate / max-pool epilogue AND the transposed aggregation in one launch, on the matrix cores, for 0/1 graphs of
// 33..128 nodes, without gate dropout:
//
//   dY[t] = d_out[t]*sg + [t = argmax_a] d_pa*ga + [t = argmax_b] d_pb*gb         models/bert_amir5.py:627-640 backwards
//   dH    = A^T . D . dY,   D = diag(1 / (rowsum(A) + 1))                           models/gcn.py:35,41 backwards (train.py:120)
//
// The tile is gate_pool_backward_tile.h (its register -> row map is also the k order of expand_mask's fragments, expand_mask.h);
// the 32-node form of this launch is gate_pool_backward_mma.hip.  One workgroup per graph, four wavefronts that walk the
// 32-column tiles w, w + 4, ....  This file's own:
//   * a tile is NB = ceil(T/32) row blocks (2..4), and the pools' winners must be known over all of them before any dY.  Pass 1
//     walks the blocks of `out` and `d_out` for the winners and d_sg.  Pass 2 reloads d_out per SOURCE block t (L2-hot: the
//     workgroup read these lines a moment ago; the scalar kernel reads d_out twice as well), forms D.dY, splits it into three bf16
//     planes (split3: residual 2^-25) and, for every DESTINATION block s whose (s, t) mask block has an edge, adds 6 MFMAs
//     (v_mfma_f32_32x32x16_bf16: 3 planes x 2 k-steps, smallest plane first) into acc[s]: NB accumulators, at most 64 registers.
//   * A^T's fragments are expanded per use: the graph's T x NB words of the TRANSPOSED row masks (ggcn_rowmask_transpose_wide,
//     once per adjacency) go to LDS once per workgroup, word-major ([t][row]: a wavefront's read is 32 consecutive words); the
//     lane of row 32 s + (lane & 31) reads word t, shifts by 4 h and calls expand_mask (12 VALU per block against 6 MFMAs of 16
//     passes each).  Blocks expanded once per workgroup into LDS would cost 16 x 2 KiB = 32 KiB (one workgroup per CU less) to
//     save those 12 instructions under MFMAs that are not the bottleneck -- this launch is bound by its three [N,F] streams; not
//     built.  A 16-bit summary (bit 4 s + t: block (s, t) has an edge), made once per workgroup by ballots, lets a wavefront skip
//     the MFMAs of an empty block: dependency arcs are short, most off-diagonal blocks of a parse are empty.
//   * 1 / (rowsum + 1) comes from `inv` (ggcn_inv_denominators: float[B*T]) through LDS, zero beyond T.
//   * no dY output and no max |dH|: an adjacency gradient keeps the two passes, and dX at these lengths is never "scaled".
//   * no form under gate dropout: ggcn_gate_pool_backward_drop + ggcn_aggregate_t keep that case.
//   * dH leaves one 32-row block at a time (store_block36).
// No atomics, a fixed summation order (blocks in ascending t, planes smallest first): bit-identical from run to run.
// Traffic per layer: out + d_out read, d_out read again (L2), dH written: 3 N F 4 bytes from memory where the two passes move 5.
// Registers (`make resources`): 207 VGPRs (the compiler keeps the loads of a block in flight next to the four accumulators), no
// scratch, 21008 bytes of LDS: two workgroups per CU (__launch_bounds__(256, 2); a bound of three spills 100 bytes per lane, of
// four 312).  rowmask_transpose_wide_kernel: 36 VGPRs, 2 KiB of LDS.
#include "expand_mask.h"
#include "gate_pool_backward_tile.h"

namespace ggcn {
namespace {

using namespace bx3;
using namespace gpb;

__global__ __launch_bounds__(256, 2) void gate_pool_backward_wide_kernel(
    const float *__restrict__ out, int64_t ldo, const float *__restrict__ store_gate, const float *__restrict__ gate_a,
    const float *__restrict__ gate_b, const float *__restrict__ d_out, int64_t ldd, const float *__restrict__ d_pa,
    const float *__restrict__ d_pb, const uint32_t *__restrict__ rowmask_t, const float *__restrict__ inv, int T, int F,
    float *__restrict__ dH, int64_t ldh, float *__restrict__ d_sg, float *__restrict__ d_ga, float *__restrict__ d_gb,
    float *__restrict__ d_bsum)
{
    __shared__ __attribute__((aligned(16))) float stage_all[4][32 * kStageLd];   // per wavefront: one 32 x 32 block of dH on its way to 16-byte stores
    __shared__ uint32_t mt[kMaxNB * kMaxT];                                      // word t of row s of A^T at [t][s]; zero beyond T
    __shared__ __attribute__((aligned(16))) float sinv[kMaxT];                   // 1 / (rowsum + 1); zero beyond T
    __shared__ uint32_t live_part[4];
    const int b = blockIdx.x;          // one workgroup per graph: its rows are ONE contiguous block of `out` / `d_out` / dH
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int nb = (T + 31) >> 5;      // 2..4 (the entry refuses anything else)
    float *stage = stage_all[wave];

    for (int i = threadIdx.x; i < kMaxNB * kMaxT; i += 256) {
        const int t = i >> 7, row = i & (kMaxT - 1);
        mt[i] = (row < T && t < nb) ? rowmask_t[((int64_t)b * T + row) * nb + t] : 0u;
    }
    if (threadIdx.x < kMaxT) sinv[threadIdx.x] = (int)threadIdx.x < T ? inv[(int64_t)b * T + threadIdx.x] : 0.0f;
    __syncthreads();
    {   // which (s, t) blocks have an edge: wavefront s looks at its 32 rows of every word
        uint32_t bits = 0u;
#pragma unroll
        for (int t = 0; t < kMaxNB; ++t)
            if (__builtin_amdgcn_ballot_w64(mt[t * kMaxT + 32 * wave + c] != 0u) != 0) bits |= 1u << t;
        if (lane == 0) live_part[wave] = bits;
    }
    __syncthreads();
    const uint32_t live = __builtin_amdgcn_readfirstlane(live_part[0] | (live_part[1] << 4) | (live_part[2] << 8) | (live_part[3] << 12));

#pragma unroll 1
    for (int col0 = wave * 32; col0 < F; col0 += 128) {   // wavefront-uniform walk over this wavefront's 32-column tiles
        const Column k = column_operands(b, col0 + c, F, store_gate, gate_a, gate_b, d_pa, d_pb);
        const GraphRows rows(out, ldo, d_out, ldd, b, T, F, h, k.colc);

        // ---- pass 1: the pools' winners over every row block, d_sg
        Winners w;
#pragma unroll 1
        for (int blk = 0; blk < nb; ++blk) {
            float ov[16], dv[16];
            rows.load(blk, ov, dv);
            scan_rows(w, k, ov, dv, blk, h, T);
        }
        exchange_halves(w);

        // ---- pass 2: per source block t, dY and D.dY in register order, then dH[s] += A^T(s, t) . (D.dY)(t) for every live s
        f32x16 acc[kMaxNB];
#pragma unroll
        for (int s = 0; s < kMaxNB; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;
        float bsum = 0.0f;
        const float pa_g = k.dpa * k.ga, pb_g = k.dpb * k.gb;
#pragma unroll 1
        for (int t = 0; t < nb; ++t) {
            float dv[16], rinv[16], gw[16];
            rows.load_d(t, dv);
            rinv_of_block(sinv, t, h, rinv);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float g = dy_row(k, w, dv[r], 32 * t + row_of(r, h), T, pa_g, pb_g);
                bsum += g;
                gw[r] = g * rinv[r];                                   // gcn.py:35: the row's own 1 / (deg + 1)
            }
            bf16x8 pl[3][2];
            split3(gw, pl);
#pragma unroll
            for (int s = 0; s < kMaxNB; ++s) {
                if (!((live >> (4 * s + t)) & 1u)) continue;   // wavefront-uniform: no edge from block t into block s (or s >= nb)
                bf16x8 af[2];
                expand_mask(mt[t * kMaxT + 32 * s + c] >> (4 * h), af);
                acc[s] = mma_01(af, pl, acc[s]);
            }
        }
        bsum += __shfl_xor(bsum, 32);
        w.acc_sg += __shfl_xor(w.acc_sg, 32);
        store_column_grads(k, w, h, bsum, d_bsum, d_sg, d_ga, d_gb);
#pragma unroll
        for (int s = 0; s < kMaxNB; ++s) {
            if (s >= nb) break;   // wavefront-uniform
            store_block36(stage, acc[s], s, dH, ldh, b, T, F, col0, lane);
        }
    }   // column tiles
}

// row masks of the transposed adjacency, graphs of 33..128 nodes (W = ceil(T/32) words per node): one workgroup per graph holds
// the graph's T x W words in LDS; thread (s, w) gathers bit s % 32 of word s / 32 of the 32 rows t = 32 w + k into word w of row
// s.  Rows of the input beyond T are never read, so bits and words at or beyond T come out 0.
__global__ __launch_bounds__(512) void rowmask_transpose_wide_kernel(const uint32_t *__restrict__ rowmask, int T,
                                                                     uint32_t *__restrict__ rowmask_t)
{
    __shared__ uint32_t m[kMaxT * kMaxNB];
    const int W = (T + 31) >> 5;
    const int64_t base = (int64_t)blockIdx.x * T * W;
    for (int i = threadIdx.x; i < T * W; i += 512) m[i] = rowmask[base + i];
    __syncthreads();
    for (int i = threadIdx.x; i < T * W; i += 512) {
        const int s = i / W, w = i - s * W;
        const int n = min(32, T - 32 * w);     // rows t = 32 w .. 32 w + n - 1 exist
        uint32_t word = 0u;
        for (int k = 0; k < n; ++k) word |= ((m[(32 * w + k) * W + (s >> 5)] >> (s & 31)) & 1u) << k;
        rowmask_t[base + i] = word;
    }
}

}  // namespace
}  // namespace ggcn

using namespace ggcn;

extern "C" {

int ggcn_rowmask_transpose_wide(const uint32_t *rowmask, int B, int T, uint32_t *rowmask_t, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_rowmask_transpose_wide";
    if (!rowmask || !rowmask_t) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (B <= 0 || T <= 0) return fail(GGCN_EINVAL, "%s: B=%d T=%d must be positive", who, B, T);
    if (T <= 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d <= 32; use ggcn_rowmask_transpose", who, T);
    if (T > kMaxT) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 128 (four words per node)", who, T);
    hipLaunchKernelGGL(rowmask_transpose_wide_kernel, dim3((unsigned)B), dim3(512), 0, st, rowmask, T, rowmask_t);
    return check_launch(who);
}

int ggcn_gate_pool_backward_wide(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                 const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const uint32_t *rowmask_t,
                                 const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *d_sg, float *d_ga, float *d_gb,
                                 float *d_bsum, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_gate_pool_backward_wide";
    if (!out || !dH || !rowmask_t || !inv) return fail(GGCN_EINVAL, "%s: null pointer", who);
    const EntryRules rules = {who, false, 33, "ggcn_gate_pool_backward_mma", kMaxT, "", true,
                              "F % 4 == 0, ldh % 4 == 0 and 16-byte aligned dH / rowmask_t; use ggcn_gate_pool_backward + ggcn_aggregate_t"};
    const int64_t ldd_in = d_out ? ldd : F;   // (no d_out: ldd is not read)
    if (const int rc = backward_entry_checks(rules, B, T, F, {ldo, ldh, ldd_in}, {ldo, ldh, ldd_in},
                                             F % 4 == 0 && ldh % 4 == 0 && aligned16(dH) && aligned16(rowmask_t)))
        return rc;
    hipLaunchKernelGGL(gate_pool_backward_wide_kernel, dim3((unsigned)B), dim3(256), 0, st, out, ldo, store_gate, gate_a, gate_b, d_out,
                       d_out ? ldd : ldo, d_pa, d_pb, rowmask_t, inv, T, F, dH, ldh, d_sg, d_ga, d_gb, d_bsum);
    return check_launch(who);
}

}  // extern "C"
