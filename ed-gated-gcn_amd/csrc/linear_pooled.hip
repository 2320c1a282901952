// The bf16x3 linear on pooled layers (ggcn_linear_pooled_layers): the BiLSTM's input projection read straight from BERT's
// layer list,
//     Y[b*R + r, f] = sum_l sum_k ( sum_c A[b,r,c] * X_l[b,c,k] ) * W[l*Dl + k, f]
// (models/bert_amir5.py:596,600,610: torch.cat, torch.bmm(transform, x) and the LSTM's x . W_ih^T).  The pooled words
// [B,R,n*Dl] are never stored: the A-operand loader of the 128 x 256 tile forms each pooled value in registers right before
// the hi / lo split.
//
// Arithmetic (what makes the launch testable): a pooled value is what pooled4 of subword_pool.hip computes -- from 0.0f, one
// fmaf per non-zero of the row of A in ascending column, an absent entry skipped (a select, never a product with a zero
// weight: a NaN in a row that no word selects does not arrive) -- and the split, the product order per k-step (lo.hi, hi.lo,
// hi.hi), the k order and the tile are those of bx3::mainloop.  So Y is bit for bit ggcn_linear(bf16x3) on the output of
// ggcn_subword_pool_layers.
//
// The loader.  A thread stages the same four rows for the whole K loop (stage_row, 8 threads a row, 16 B of k each), so a
// prologue compacts the entry list of each of the tile's 128 rows ONCE (ballot + popcount over the dense row of A, ascending
// column) into LDS: the first kCap (column, value) pairs and the full count.  Per 32-deep stage the layer is uniform
// (Dl % 32 == 0).  The rows of X of a row's first kFast = 4 entries are requested unconditionally, as the loop of bf16x3_core.h
// requests its rows of X (clamped address, no predicate; an absent entry reads sub-word row 0 of its sentence and the select on
// the entry count is applied at the split).  Four entries of all four passes would be 64 registers in flight beside 128
// accumulators, so the requests run HALF a stage ahead in a ring of two passes (32 registers): the staging is spread over both
// k-steps of the stage, one pass pooled and split after every second MFMA block, and the pass two further on requested into
// the registers it freed.  A row with more than four entries adds the others at the split with loads of its own, from the LDS
// list up to kCap and from a re-scan of the dense row of A beyond it: slower, the same bits, no refusal.
#include "bf16x3_core.h"

namespace ggcn {
namespace {

using namespace bx3;

static_assert(RN == 2 && BM == 128, "written for the 128 x 256 tile of four wavefronts side by side");

constexpr int kMaxCols = 2048;  // columns of A (as ggcn_subword_pool_layers)
constexpr int kFast = 4;        // entries per row whose rows of X are requested ahead, unconditionally
constexpr int kSlots = 2;       // passes whose requests are in flight: half a stage ahead
constexpr int kCap = 8;         // entries per row kept in LDS
constexpr int kOffIdx = kLdsBytes;                      // int   [BM][kCap]
constexpr int kOffVal = kOffIdx + BM * kCap * 4;        // float [BM][kCap]
constexpr int kOffCnt = kOffVal + BM * kCap * 4;        // int   [BM]
constexpr int kOffRow = kOffCnt + BM * 4;               // int64 [BM][kFast]: where the first entries' rows of X start in a layer
constexpr int kOffSent = kOffRow + BM * kFast * 8;      // int64 [BM][2]: where the row's sentence starts in a layer, and its row of A
constexpr int kPooledLdsBytes = kOffSent + BM * 2 * 8;

struct LayerPtrs {
    const float *p[GGCN_POOL_MAX_LAYERS];
};

__device__ __forceinline__ float4 fma4(float v, const float4 &x, const float4 &a)
{
    return make_float4(fmaf(v, x.x, a.x), fmaf(v, x.y, a.y), fmaf(v, x.z, a.z), fmaf(v, x.w, a.w));
}
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

__global__ __launch_bounds__(kThreads, kWavesPerSimd) void linear_pooled_kernel(
    const float *__restrict__ A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const LayerPtrs layers, int64_t x_batch, int64_t ldx,
    const char *__restrict__ wpack, float *__restrict__ Y, int64_t ldy, int64_t M, int R, int C, int Dl, int K, int F,
    int m_tiles, int n_wg, int k_steps)
{
    __shared__ __attribute__((aligned(16))) char lds[kPooledLdsBytes];
    int m_tile, n_wgi;
    if (!tile_of_block(blockIdx.x, m_tiles, n_wg, m_tile, n_wgi)) return;  // before any barrier

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wn = wave % WN;
    const int64_t m0 = (int64_t)m_tile * BM;
    const int n_tiles_total = (F + NT - 1) / NT;
    const int nt0 = n_wgi * (BN / NT) + wn * RN;  // this wavefront's first 32-column tile
    int *e_idx = reinterpret_cast<int *>(lds + kOffIdx);
    float *e_val = reinterpret_cast<float *>(lds + kOffVal);
    int *e_cnt = reinterpret_cast<int *>(lds + kOffCnt);
    int64_t *e_row = reinterpret_cast<int64_t *>(lds + kOffRow);
    int64_t *e_sent = reinterpret_cast<int64_t *>(lds + kOffSent);

    // rows past M are clamped to row M-1: a row only feeds the same row of Y, never stored
    auto row_of = [&](int row, int &b, int &r) {
        const int64_t gm = m0 + row;
        const int g = (int)(gm < M ? gm : M - 1);   // (M <= INT32_MAX: a 32-bit division)
        b = g / R;
        r = g - b * R;
    };

    // ---- prologue: the entry list of every row of the tile, once.  A wavefront takes four rows at a time (their loads in
    // flight together), 64 columns a round.
    for (int rg = 0; rg < BM / 16; ++rg) {
        const float *ar[4];
        int total[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int b, r;
            row_of(rg * 16 + wave * 4 + j, b, r);
            ar[j] = A + b * sa_b + r * sa_r;
            total[j] = 0;
        }
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int c = c0 + lane;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = c < C ? ar[j][c * sa_c] : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = rg * 16 + wave * 4 + j;
                const bool nz = v[j] != 0.0f;
                const unsigned long long m = __ballot(nz);
                const int pos = total[j] + __popcll(m & ((1ull << lane) - 1ull));
                if (nz && pos < kCap) {
                    e_idx[row * kCap + pos] = c;
                    e_val[row * kCap + pos] = v[j];
                }
                total[j] += __popcll(m);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e_cnt[rg * 16 + wave * 4 + j] = total[j];
        }
    }
    __syncthreads();

    static_assert(Geom<float>::NP == 4 && Geom<float>::TPR == 8, "four passes of 32 rows, 8 threads a row");
    const int s_k = (tid % Geom<float>::TPR) * 4;  // first k of this thread's 16-B piece
    // element offset of each fast entry's row of X inside a layer: kept in LDS like the counts (read back per stage: the 64-bit
    // offsets of four rows do not fit the register file next to the accumulators)
    if (tid < BM) {
        int b, r;
        row_of(tid, b, r);
#pragma unroll
        for (int f = 0; f < kFast; ++f) {
            const int c = f < e_cnt[tid] ? e_idx[tid * kCap + f] : 0;   // an absent entry: a valid row, its values unselected
            e_row[tid * kFast + f] = (int64_t)b * x_batch + (int64_t)c * ldx;
        }
        e_sent[tid * 2] = (int64_t)b * x_batch;
        e_sent[tid * 2 + 1] = b * sa_b + r * sa_r;
    }
    __syncthreads();

    // the stage that starts at k0 lies in one layer: its base, advanced to the stage's first column
    auto stage_base = [&](int k0) -> const float * {
        const int l = k0 / Dl;
        return layers.p[l] + (k0 - l * Dl);
    };

    float4 ra[kSlots][kFast];
    auto load_a_pass = [&](int i, int slot, const float *xs) {
#pragma unroll
        for (int f = 0; f < kFast; ++f) ra[slot][f] = ld4(xs + e_row[stage_row<float>(i) * kFast + f] + s_k);
    };
    // the entries past kFast of pass i's row, added in ascending column with loads of their own
    auto more_entries = [&](int i, float4 p, int k0) -> float4 {
        const int row = stage_row<float>(i);
        const float *xb = stage_base(k0) + e_sent[row * 2] + s_k;
        const int n = e_cnt[row] < kCap ? e_cnt[row] : kCap;
        int e = kFast;
        for (; e + 1 < n; e += 2) {   // two rows in flight
            const float4 x0 = ld4(xb + (int64_t)e_idx[row * kCap + e] * ldx);
            const float4 x1 = ld4(xb + (int64_t)e_idx[row * kCap + e + 1] * ldx);
            p = fma4(e_val[row * kCap + e], x0, p);
            p = fma4(e_val[row * kCap + e + 1], x1, p);
        }
        if (e < n) p = fma4(e_val[row * kCap + e], ld4(xb + (int64_t)e_idx[row * kCap + e] * ldx), p);
        if (e_cnt[row] > kCap) {   // beyond the list: the dense row of A again, from the column after the last one kept
            const float *arow = A + e_sent[row * 2 + 1];
            for (int c = e_idx[row * kCap + kCap - 1] + 1; c < C; ++c) {
                const float v = arow[c * sa_c];
                if (v != 0.0f) p = fma4(v, ld4(xb + (int64_t)c * ldx), p);
            }
        }
        return p;
    };
    // pool pass i (rows of the stage that starts at k0) and split it into the two bf16 planes of buffer `buf`
    auto store_a_pass = [&](int buf, int i, int slot, int k0) {
        char *hi_plane = lds + buf * (2 * BM * ROWB);
        char *lo_plane = hi_plane + BM * ROWB;
        const int row = stage_row<float>(i);
        const int off = a_lds_off(row, s_k >> 3) + (s_k & 4) * 2;
        const int n_row = e_cnt[row];
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int f = 0; f < kFast; ++f) {
            const float4 t = fma4(e_val[row * kCap + f], ra[slot][f], p);
            const bool in = f < n_row;
            p = make_float4(in ? t.x : p.x, in ? t.y : p.y, in ? t.z : p.z, in ? t.w : p.w);
        }
        if (n_row > kFast) p = more_entries(i, p, k0);
        const float x[4] = {p.x, p.y, p.z, p.w};
        __bf16 hi[4], lo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            hi[c] = (__bf16)x[c];
            lo[c] = (__bf16)(x[c] - (float)hi[c]);
        }
        *reinterpret_cast<bf16x4 *>(hi_plane + off) = bf16x4{hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<bf16x4 *>(lo_plane + off) = bf16x4{lo[0], lo[1], lo[2], lo[3]};
    };

    // B fragments straight from the packed image; indices clamped, never predicated: a column
    // tile past F duplicates the last real tile and is never stored.
    const char *bbase[RN];
#pragma unroll
    for (int j = 0; j < RN; ++j) {
        const int ntc = nt0 + j < n_tiles_total ? nt0 + j : n_tiles_total - 1;
        bbase[j] = wpack + ((int64_t)ntc * k_steps) * 2 * FRAG_BYTES + lane * 16;
    }
    auto load_b = [&](int ks, bf16x8 (&b)[RN][2]) {  // [col tile][plane]
        ks = ks < k_steps ? ks : k_steps - 1;        // the one-step-ahead prefetch of the last stage
        const int64_t o = (int64_t)ks * 2 * FRAG_BYTES;
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            b[j][0] = *reinterpret_cast<const bf16x8 *>(bbase[j] + o);
            b[j][1] = *reinterpret_cast<const bf16x8 *>(bbase[j] + o + FRAG_BYTES);
        }
    };

    f32x16 acc[4][RN];
    const int f_row = lane & 31;
    const int f_half = lane >> 5;
    // one 32-row block of one k-step: 2 LDS fragment reads + 6 MFMAs, in the product order of bx3::mainloop
    auto mma_block = [&](int buf, int s, int i, const bf16x8 (&b)[RN][2]) {
        __builtin_amdgcn_iglp_opt(0);
        const char *hi_plane = lds + buf * (2 * BM * ROWB);
        const char *lo_plane = hi_plane + BM * ROWB;
        const int off = a_lds_off(f_row + i * 32, s * 2 + f_half);
        const bf16x8 a_hi = *reinterpret_cast<const bf16x8 *>(hi_plane + off);
        const bf16x8 a_lo = *reinterpret_cast<const bf16x8 *>(lo_plane + off);
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b[j][0], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b[j][1], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b[j][0], acc[i][j], 0, 0, 0);
        }
    };

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    bf16x8 b0[RN][2], b1[RN][2];
    const int stages = K / BK;
    const int last_k0 = (stages - 1) * BK;

    // ---- prologue: stage 0 pooled and split into buffer 0, two passes at a time; the first two passes of stage 1 in flight ----
    {
        const float *xs = stage_base(0);
        load_a_pass(0, 0, xs);
        load_a_pass(1, 1, xs);
        load_b(0, b0);
        store_a_pass(0, 0, 0, 0);
        store_a_pass(0, 1, 1, 0);
        load_a_pass(2, 0, xs);
        load_a_pass(3, 1, xs);
        store_a_pass(0, 2, 0, 0);
        store_a_pass(0, 3, 1, 0);
        xs = stage_base(BK < last_k0 ? BK : last_k0);
        load_a_pass(0, 0, xs);
        load_a_pass(1, 1, xs);
    }
    __syncthreads();

    // ---- the stage of bx3::mainloop, with the staging spread over both k-steps: after every second MFMA block one pass of the
    // NEXT stage is pooled and split into the other buffer, and the rows of the pass two further on are requested into the
    // registers it freed (half a stage ahead); B fragments one k-step ahead.  Every global load sits between MFMAs.
    auto stage = [&](int st, auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        const int k_next1 = (st + 1) * BK < last_k0 ? (st + 1) * BK : last_k0;
        const int k_next2 = (st + 2) * BK;
        const int ka = k_next2 < last_k0 ? k_next2 : last_k0;  // past the end: harmless re-read
        const float *xs1 = stage_base(k_next1), *xs2 = stage_base(ka);
        auto unit = [&](auto jc) {     // pass j of stage st+1 out of its slot, then the pass two further on into it
            constexpr int j = decltype(jc)::value;
            store_a_pass(buf ^ 1, j, j & 1, k_next1);
            if constexpr (j < 2) load_a_pass(j + 2, j & 1, xs1);
            else load_a_pass(j - 2, j & 1, xs2);
        };
        load_b(st * KS + 1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 0, 0, b0);
        unit(std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 0, 1, b0);
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 0, 2, b0);
        unit(std::integral_constant<int, 1>{});
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 0, 3, b0);
        load_b(st * KS + 2, b0);
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 1, 0, b1);
        unit(std::integral_constant<int, 2>{});
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 1, 1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 1, 2, b1);
        unit(std::integral_constant<int, 3>{});
        __builtin_amdgcn_sched_barrier(0);
        mma_block(buf, 1, 3, b1);
        __syncthreads();  // the only barrier of the stage
    };
    int st = 0;
    for (; st + 1 < stages; st += 2) {
        stage(st, std::integral_constant<int, 0>{});
        stage(st + 1, std::integral_constant<int, 1>{});
    }
    if (st < stages) stage(st, std::integral_constant<int, 0>{});

    // ---- fp32 output as 16-byte row stores, staged through the (idle) A buffers: the epilogue of linear_split.hip ----
    const bool full_rows = m0 + BM <= M;  // workgroup-uniform: the row guard only exists in the last tile
    float *stage_lds = reinterpret_cast<float *>(lds) + wave * (32 * 64);
    const int c = lane & 31, h = lane >> 5;
    const int colq = (lane & 15) * 4;
    const int gcol = nt0 * NT + colq;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row0 = (r & 3) + 8 * (r >> 2);
                stage_lds[(row0 + 4 * h) * 64 + ((32 * j + c) ^ (32 * h))] = acc[i][j][r];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int64_t gm0 = m0 + i * 32;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = 4 * it + (lane >> 4);
            const float4 v4 = *reinterpret_cast<const float4 *>(&stage_lds[row * 64 + (colq ^ (32 * ((row >> 2) & 1)))]);
            if ((full_rows || gm0 + row < M) && gcol < F)
                *reinterpret_cast<float4 *>(Y + (gm0 + row) * ldy + gcol) = v4;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace
}  // namespace ggcn

using namespace ggcn;

extern "C" {

// 1 = the launch is taken, -ggcn_status (message set) where ggcn_linear_pooled_layers refuses.  Host only: reads the n_layers
// entries of `layers` and nothing behind any device pointer.  The launcher dispatches on this answer.
int ggcn_linear_pooled_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                                   int64_t x_batch, int64_t ldx, const void *wpack, const float *Y, int64_t ldy, int B, int R, int C,
                                   int Dl, int F)
{
    const char *who = "ggcn_linear_pooled_layers";
    (void)sa_b; (void)sa_r; (void)sa_c;
    if (!A || !layers || !wpack || !Y) return -fail(GGCN_EINVAL, "%s: null pointer", who);
    if (n_layers < 1) return -fail(GGCN_EINVAL, "%s: n_layers=%d must be positive", who, n_layers);
    if (n_layers > GGCN_POOL_MAX_LAYERS)
        return -fail(GGCN_EUNSUPPORTED, "%s: n_layers=%d > %d layers a launch", who, n_layers, GGCN_POOL_MAX_LAYERS);
    for (int l = 0; l < n_layers; ++l)
        if (!layers[l]) return -fail(GGCN_EINVAL, "%s: layers[%d] is a null pointer", who, l);
    if (B <= 0 || R <= 0 || C <= 0 || Dl <= 0 || F <= 0)
        return -fail(GGCN_EINVAL, "%s: B=%d R=%d C=%d Dl=%d F=%d must be positive", who, B, R, C, Dl, F);
    if (C > kMaxCols) return -fail(GGCN_EUNSUPPORTED, "%s: C=%d > %d columns", who, C, kMaxCols);
    if ((int64_t)B * R > (int64_t)INT32_MAX) return -fail(GGCN_EUNSUPPORTED, "%s: too many rows", who);
    if (ldx < Dl || ldy < F) return -fail(GGCN_EINVAL, "%s: leading dimension too small", who);
    if (reinterpret_cast<uintptr_t>(A) % 4 || reinterpret_cast<uintptr_t>(Y) % 4)
        return -fail(GGCN_EINVAL, "%s: A or Y not aligned to its element", who);
    for (int l = 0; l < n_layers; ++l)
        if (reinterpret_cast<uintptr_t>(layers[l]) % 4)
            return -fail(GGCN_EINVAL, "%s: layers[%d] not aligned to its element", who, l);
    if (!aligned16(wpack)) return -fail(GGCN_EINVAL, "%s: wpack must be 16-byte aligned", who);
    const int64_t k_steps = ((int64_t)n_layers * Dl + BK - 1) / BK * (BK / KSTEP);
    if (k_steps > 65535) return -fail(GGCN_EUNSUPPORTED, "%s: K=n_layers*Dl=%lld too large for ggcn_weight_pack", who, (long long)n_layers * Dl);
    bool form = (Dl % BK == 0) && (ldx % 4 == 0) && (x_batch % 4 == 0) && (F % 4 == 0) && (ldy % 4 == 0) && aligned16(Y);
    for (int l = 0; l < n_layers; ++l) form = form && aligned16(layers[l]);
    if (!form)
        return -fail(GGCN_EUNSUPPORTED, "%s: needs Dl %% 32 == 0, ldx, x_batch, F and ldy multiples of 4 and 16-byte aligned layers and Y "
                                        "(use ggcn_subword_pool_layers, then ggcn_linear with GGCN_PREC_BF16X3)", who);
    if (linear_split_grid((int64_t)B * R, F) > (int64_t)INT32_MAX) return -fail(GGCN_EUNSUPPORTED, "%s: too many workgroups", who);
    return 1;
}

int ggcn_linear_pooled_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                              int64_t x_batch, int64_t ldx, const void *wpack, float *Y, int64_t ldy, int B, int R, int C, int Dl,
                              int F, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const int form = ggcn_linear_pooled_layers_form(A, sa_b, sa_r, sa_c, layers, n_layers, x_batch, ldx, wpack, Y, ldy, B, R, C, Dl, F);
    if (form < 0) return -form;
    LayerPtrs ptrs = {};
    for (int l = 0; l < n_layers; ++l) ptrs.p[l] = static_cast<const float *>(layers[l]);
    const int64_t M = (int64_t)B * R;
    const int K = n_layers * Dl;
    const int k_steps = K / KSTEP;
    const int64_t m_tiles = (M + BM - 1) / BM;
    const int n_wg = (F + BN - 1) / BN;
    const int64_t grid = linear_split_grid(M, F);
    hipLaunchKernelGGL(linear_pooled_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, A, sa_b, sa_r, sa_c, ptrs, x_batch, ldx,
                       static_cast<const char *>(wpack), Y, ldy, M, R, C, Dl, K, F, (int)m_tiles, n_wg, k_steps);
    return check_launch("ggcn_linear_pooled_layers");
}

}  // extern "C"
