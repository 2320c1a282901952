// Gradient of the layer with respect to a REAL-VALUED adjacency (models/gcn.py:33-45 is ordinary ATen: a soft or learned
// `adj` gets its gradient from autograd there).  For one graph, y = D.A.H + b with H = X.W, D = diag(inv),
// inv_i = 1 / (sum_k A_ik + 1), and dY the gradient at y:
//
//     G_ij  = inv_i * (dY_i . H_j)              T x T per graph, reduction over F
//     c_i   = inv_i * sum_k A_ik * G_ik         (the row's non-zeros: the derivative of the denominator)
//     dA_ij = G_ij - c_i                        for EVERY (i, j), edges and non-edges alike
//
// G = dY.H^T is an "NT" product: both operands are contiguous along the reduction axis F, so the MFMA fragments of either are
// consecutive floats of one row -- read straight from global memory (16-byte loads, or elements for rows that are not
// 16-byte aligned), split into bf16 hi / lo in registers (gradients have no range contract: bf16 keeps the fp32 exponent), and
// multiplied as hi.hi + lo.hi + hi.lo on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (bf16x3_core.h).
//
// Mapping: workgroup = (graph, block of 32 rows i) x ALL T columns; its 1..4 wavefronts share the 32-column blocks (wavefront w
// owns blocks w, w + nw, ...: at most 4 each up to T = 512) and keep one accumulator tile per block, so a dY fragment is loaded and
// split once per wavefront.  The scaled 32 x T block of G goes to LDS (64 KiB at T = 512), c_i is summed from the CSR
// row out of LDS (lanes stride the row's edges, then a fixed butterfly), and every d_adj row is written once, with 16-byte stores
// when T % 4 == 0.  Graphs of <= 32 nodes have a single column block: there the four wavefronts share F (32 columns each in turn)
// and their partial tiles are added in LDS in wavefront order.  One launch, no atomics, a fixed summation order: bit-reproducible; no workgroup depends on another.
// Rows i >= T of the last row block and columns j >= T of the last column block belong to the next graph (or to nothing): their
// addresses are clamped into the graph, their fragments zeroed, and they are never stored.  The F tail of the last k-step reads
// zeros, not the pad columns.
#include "common.h"
#include "bf16x3_core.h"

namespace ggcn {
namespace {

using bx3::bf16x8;
using bx3::f32x16;

constexpr int kRows = 32;      // rows of G per workgroup = one MFMA tile

// 16 consecutive floats of `row` from column k (k % 16 == 0), raw: columns >= F re-read column 0 and are zeroed in the split
template <bool VEC>
__device__ __forceinline__ void load_raw(const float *__restrict__ row, int k, int F, float (&v)[16])
{
    if constexpr (VEC) {   // 16-byte aligned rows, F % 4 == 0: a float4 that starts below F ends below F
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kk = k + 4 * q;
            const float4 t = *reinterpret_cast<const float4 *>(row + (kk < F ? kk : 0));
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] = row[k + c < F ? k + c : 0];
    }
}

// the 16 floats as two fragments of bf16 hi / lo; columns >= F and a dead row read as zeros
__device__ __forceinline__ void split(const float (&v)[16], int k, int F, bool live, bf16x8 (&hi)[2], bf16x8 (&lo)[2])
{
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float x = (live && k + c < F) ? v[c] : 0.0f;
        const __bf16 t = (__bf16)x;
        hi[c >> 3][c & 7] = t;
        lo[c >> 3][c & 7] = (__bf16)(x - (float)t);
    }
}

// NCB: 32-column blocks per wavefront (1 up to T = 128, 2 up to 256, 4 up to 512)
template <bool VEC, int NCB>
__global__ __launch_bounds__(256) void adjacency_grad_kernel(
    const float *__restrict__ dY, int64_t ldy, const float *__restrict__ hidden, int64_t ldh, const float *__restrict__ inv,
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const float *__restrict__ vals, int T, int F,
    int n_rb, int n_cb, float *__restrict__ d_adj, bool store_vec, bool k_split)
{
    extern __shared__ float s_g[];           // [32][n_cb * 32] scaled G (k_split: one such slab per wavefront)
    const int ldg = n_cb * 32;
    const int b = blockIdx.x / n_rb;
    const int i0 = (blockIdx.x - b * n_rb) * kRows;
    const int nw = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const int64_t node0 = (int64_t)b * T;

    // ---- G block on the matrix cores.  The sum over k may run in any order as long as both operands agree on it: per 32 columns
    // of F, lane (r, h) holds the 16 CONSECUTIVE floats k0 + 16 h .. + 15 of its row (64 contiguous bytes, the two halves of a
    // 128-byte line between h = 0 and 1) -- elements 0..7 feed the first MFMA k-step, 8..15 the second.  The raw loads of the
    // next 32 columns are issued before the split and the MFMAs of the current ones.
    const bool a_live = i0 + r < T;
    const float *a_row = dY + (node0 + (a_live ? i0 + r : 0)) * ldy;
    const float *b_row[NCB];
    bool b_live[NCB];
    int my_cb = 0;
    // k_split (graphs of <= 32 nodes, one column block): the wavefronts share F instead, 32 columns at a time in turn
    const int wcol = k_split ? 0 : wave, ncolw = k_split ? 1 : nw;
    const int kb = k_split ? 32 * wave : 0, kstep = k_split ? 32 * nw : 32;
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
        const int cb = wcol + c * ncolw;
        const int j = cb * 32 + r;
        b_live[c] = cb < n_cb && j < T;
        b_row[c] = hidden + (node0 + (b_live[c] ? j : 0)) * ldh;
        if (cb < n_cb) my_cb = c + 1;
    }
    f32x16 acc[NCB];
#pragma unroll
    for (int c = 0; c < NCB; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[c][q] = 0.0f;
    float ra[16], rb[NCB][16];
    load_raw<VEC>(a_row, kb + 16 * h, F, ra);
#pragma unroll
    for (int c = 0; c < NCB; ++c) load_raw<VEC>(b_row[c], kb + 16 * h, F, rb[c]);
    for (int k0 = kb; k0 < F; k0 += kstep) {
        const int k = k0 + 16 * h;
        const int kn = k0 + kstep < F ? k + kstep : k;   // past the end: a harmless re-read
        float na[16], nb[NCB][16];
        load_raw<VEC>(a_row, kn, F, na);
#pragma unroll
        for (int c = 0; c < NCB; ++c) load_raw<VEC>(b_row[c], kn, F, nb[c]);
        bf16x8 a_hi[2], a_lo[2];
        split(ra, k, F, a_live, a_hi, a_lo);
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
            if (c < my_cb) {   // wavefront-uniform
                bf16x8 b_hi[2], b_lo[2];
                split(rb[c], k, F, b_live[c], b_hi, b_lo);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo[s2], b_hi[s2], acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi[s2], b_lo[s2], acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi[s2], b_hi[s2], acc[c], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) ra[q] = na[q];
#pragma unroll
        for (int c = 0; c < NCB; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) rb[c][q] = nb[c][q];
    }
    // C layout: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float inv_r[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
        inv_r[q] = i0 + row < T ? inv[node0 + i0 + row] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
        if (c < my_cb) {
            const int col = (wcol + c * ncolw) * 32 + r + (k_split ? wave * kRows * ldg : 0);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
                s_g[row * ldg + col] = acc[c][q] * inv_r[q];
            }
        }
    }
    __syncthreads();
    if (k_split) {   // the wavefronts' partial tiles, added in wavefront order into the first slab
        for (int idx = threadIdx.x; idx < kRows * ldg; idx += blockDim.x) {
            float g = s_g[idx];
            for (int w = 1; w < nw; ++w) g += s_g[w * kRows * ldg + idx];
            s_g[idx] = g;
        }
        __syncthreads();
    }

    // ---- per row (wavefront w owns rows w, w + nw, ...): c_i = inv_i * sum_e A_ie * G_ie over the row's non-zeros (global column
    // ids: local = id - b*T), lanes striding the edges and a fixed butterfly after which every lane holds the sum; then the row of
    // d_adj, written once
    for (int row = wave; row < kRows; row += nw) {
        const int i = i0 + row;
        if (i >= T) break;   // wavefront-uniform
        const float *g_row = s_g + row * ldg;
        const int e0 = rowptr[node0 + i], e1 = rowptr[node0 + i + 1];
        float s = 0.0f;
        for (int e = e0 + lane; e < e1; e += 64) {
            const int j = colidx[e] - (int)node0;
            const float g = (j >= 0 && j < T) ? g_row[j] : 0.0f;
            s = fmaf(vals ? vals[e] : 1.0f, g, s);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        const float c = s * inv[node0 + i];
        float *out = d_adj + (node0 + i) * (int64_t)T;
        if (store_vec) {   // T % 4 == 0 and a 16-byte aligned d_adj: every row starts on 16 bytes
            for (int j = lane * 4; j < T; j += 256) {
                const float4 g = *reinterpret_cast<const float4 *>(g_row + j);
                *reinterpret_cast<float4 *>(out + j) = make_float4(g.x - c, g.y - c, g.z - c, g.w - c);
            }
        } else {
            for (int j = lane; j < T; j += 64) out[j] = g_row[j] - c;
        }
    }
}

}  // namespace
}  // namespace ggcn

using namespace ggcn;

extern "C" {

int ggcn_adjacency_grad(const float *dY, int64_t ldy, const float *hidden, int64_t ldh, const float *inv, const int32_t *rowptr,
                        const int32_t *colidx, const float *vals, int B, int T, int F, float *d_adj, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_adjacency_grad";
    if (!dY) return fail(GGCN_EINVAL, "%s: dY is NULL", who);
    if (!hidden) return fail(GGCN_EINVAL, "%s: hidden is NULL", who);
    if (!inv) return fail(GGCN_EINVAL, "%s: inv is NULL", who);
    if (!rowptr) return fail(GGCN_EINVAL, "%s: rowptr is NULL", who);
    if (!colidx) return fail(GGCN_EINVAL, "%s: colidx is NULL", who);
    if (!d_adj) return fail(GGCN_EINVAL, "%s: d_adj is NULL", who);
    if (B < 0) return fail(GGCN_EINVAL, "%s: B=%d is negative", who, B);
    if (T < 1) return fail(GGCN_EINVAL, "%s: T=%d must be at least 1", who, T);
    if (F < 1) return fail(GGCN_EINVAL, "%s: F=%d must be at least 1", who, F);
    if (ldy < F) return fail(GGCN_EINVAL, "%s: ldy=%lld < F=%d", who, (long long)ldy, F);
    if (ldh < F) return fail(GGCN_EINVAL, "%s: ldh=%lld < F=%d", who, (long long)ldh, F);
    const struct { const void *p; const char *name; } ptrs[] = {{dY, "dY"}, {hidden, "hidden"}, {inv, "inv"}, {rowptr, "rowptr"},
                                                                 {colidx, "colidx"}, {vals, "vals"}, {d_adj, "d_adj"}};
    for (const auto &a : ptrs)
        if (reinterpret_cast<uintptr_t>(a.p) & 3u) return fail(GGCN_EINVAL, "%s: %s not 4-byte aligned", who, a.name);
    if (T > GGCN_LONG_MAX_T)
        return fail(GGCN_EUNSUPPORTED, "%s: T=%d > GGCN_LONG_MAX_T=%d (the 32 x T block of G is kept in LDS)", who, T, GGCN_LONG_MAX_T);
    if (B == 0) return GGCN_OK;
    const int n_rb = (T + kRows - 1) / kRows, n_cb = (T + 31) / 32;
    const int64_t blocks = (int64_t)B * n_rb;
    if (blocks > 0x7fffffffLL) return fail(GGCN_EUNSUPPORTED, "%s: B*ceil(T/32)=%lld workgroups exceed the grid", who, (long long)blocks);
    // graphs of <= 32 nodes have one column block: four wavefronts share F instead (partial tiles added in LDS in a fixed order),
    // which fills the SIMDs where one wavefront per graph leaves a third of a round empty (4096 x 32 x 768: 247 -> see DESIGN.md 4.7)
    const bool k_split = n_cb == 1 && F > 32;
    const int nw = k_split ? 4 : (n_cb < 4 ? n_cb : 4);
    const size_t lds = (size_t)kRows * n_cb * 32 * sizeof(float) * (k_split ? nw : 1);   // 64 KiB at T = 512
    const bool vec = aligned16(dY) && aligned16(hidden) && ldy % 4 == 0 && ldh % 4 == 0 && F % 4 == 0;   // (F % 4: no float4 past a row's F)
    const bool store_vec = T % 4 == 0 && aligned16(d_adj);
    const int ncb = k_split ? 1 : (n_cb + nw - 1) / nw;   // column blocks per wavefront: 1 up to T = 128, 2 up to 256, 3 or 4 beyond
    auto kern = ncb == 1 ? (vec ? adjacency_grad_kernel<true, 1> : adjacency_grad_kernel<false, 1>)
              : ncb == 2 ? (vec ? adjacency_grad_kernel<true, 2> : adjacency_grad_kernel<false, 2>)
                         : (vec ? adjacency_grad_kernel<true, 4> : adjacency_grad_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * nw), lds, st, dY, ldy, hidden, ldh, inv, rowptr, colidx, vals, T, F,
                       n_rb, n_cb, d_adj, store_vec, k_split);
    return check_launch(who);
}

}  // extern "C"
