// The recurrence of the classifier's BiLSTM (models/bert_amir5.py:557,610: nn.LSTM(9216, 128, bidirectional, batch_first, one layer)) in
// inference, as ONE launch over all T steps and both directions.  The input projection G = X.[W_ih_f ; W_ih_r]^T is the library's
// own ggcn_linear (bf16x3) and is handed in; this file owns the T dependent steps
//     a = G[b*T+t, d*4hd:(d+1)*4hd] + bias_d + h.Whh_d^T      i, f, o = sigmoid(a[0:hd]), sigmoid(a[hd:2hd]), sigmoid(a[3hd:4hd])
//     g = tanh(a[2hd:3hd])        c = f*c + i*g        h = o*tanh(c)        Y[b*T+t, d*hd:(d+1)*hd] = h
// with h0 = c0 = 0, t ascending for d = 0 and descending for d = 1 (PyTorch's gate order i, f, g, o).
//
// Form: exact fp32 on the VALU.  grid (ceil(B / 16), 2 directions), 512 threads.  Thread j owns gate column j of its direction:
// the 128 weights Whh_d[j, :] stay in its registers for the whole launch (one direction is 256 KiB: more than the LDS), the h of
// the tile's 16 sentences sits in LDS and is read as broadcast 16-byte reads (every lane the same address), so a step is
// 16 x 128 FMAs per thread.  The activated gates meet in LDS; thread (u, s mod 4) then updates the cells (s, u), whose c lives in
// its registers: h and c never leave the chip.  The G rows of step t+1 are requested before step t's arithmetic.  Every sum is
// one FMA chain, k ascending, that starts from G + bias: no atomics, the same bits on every call, for a sentence wherever it
// sits in a tile or a batch, and the two directions run the same instructions.
//
// Training (ggcn_bilstm_recurrence_save, ggcn_bilstm_recurrence_backward): the saving forward is the same step body with three
// stores added (the activated gates over G's own element, c after the step, the h the step read), so its Y is the plain kernel's
// bit for bit.  The backward is the forward's mirror, again ONE launch over all T steps and both directions, each direction's time
// walked backwards: thread (k = j & 127, q = j >> 7) keeps the COLUMN Whh_d[q*128 .. q*128+127, k] in registers, the tile's
// da = dL/da sits in LDS as [s][4hd] and is read as broadcast 16-byte reads in the forward's paced pieces, the four partial sums
// of dh_rec = da . Whh_d meet in LDS and are added in the order q = 0, 1, 2, 3; dc and dh_rec never leave the chip, and the loads
// of the next step walked (gates, C, dY) are requested before this step's arithmetic.
#include "common.h"

namespace ggcn {
namespace {

constexpr int kHd = 128, kCols = 4 * kHd, kSent = GGCN_BILSTM_TILE, kLstmThreads = kCols;
constexpr int kPieces = (kHd / 4) * (kSent / 4);
static_assert(kSent % 4 == 0, "four cell groups share a tile's sentences");

// 0 / 1 for |v| ~ 1e4 without a NaN: expf(-v) overflows to +inf on the negative side (1 / inf = 0) and is 0 on the positive one
__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

// The step body of both forward kernels.  SAVE adds three stores per step and nothing else: gates [B*T, ldg] (may be G itself: a
// thread overwrites the one element it has read, and the rows of step t + 1 are read before those of step t are written), C and
// Hprev [B*T, 2hd] contiguous.
template <bool SAVE>
__device__ __forceinline__ void bilstm_recurrence_body(const float *G, int64_t ldg, const float *__restrict__ Whh_f,
                                                       const float *__restrict__ Whh_r, const float *__restrict__ bias_f,
                                                       const float *__restrict__ bias_r, float *__restrict__ Y, int64_t ldy, int B, int T,
                                                       float *gates, float *__restrict__ C, float *__restrict__ Hprev)
{
    __shared__ __attribute__((aligned(16))) float h_lds[kSent * kHd];   // h of the tile's sentences: [s][k]
    __shared__ float act[kSent * kCols];                                 // the activated gates of this step: [s][j]
    const int j = threadIdx.x, d = blockIdx.y, b0 = blockIdx.x * kSent;
    const float *__restrict__ whh = (d ? Whh_r : Whh_f) + (int64_t)j * kHd;
    const float *__restrict__ bias = d ? bias_r : bias_f;
    float w[kHd];
#pragma unroll
    for (int k = 0; k < kHd; k += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(whh + k);
        w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
    }
    const float bj = bias ? bias[j] : 0.0f;
    const bool is_tanh = (j >> 7) == 2;                 // (uniform per wavefront: a gate is two wavefronts wide)
    const int u = j & (kHd - 1), sg = j >> 7;           // the cells this thread updates: (s = sg + 4 m, u)
    float c[kSent / 4];
#pragma unroll
    for (int m = 0; m < kSent / 4; ++m) c[m] = 0.0f;
    for (int i = j; i < kSent * kHd; i += kLstmThreads) h_lds[i] = 0.0f;

    // a sentence past B reads the batch's last sentence (its results are dropped): every offset below is uniform but j
    const float *gcol = G + d * kCols + j;
    float gn[kSent];
    {
        const int t = d ? T - 1 : 0;
#pragma unroll
        for (int s = 0; s < kSent; ++s) {
            const int b = b0 + s < B ? b0 + s : B - 1;
            gn[s] = gcol[((int64_t)b * T + t) * ldg];
        }
    }
    __syncthreads();
    for (int step = 0; step < T; ++step) {
        const int t = d ? T - 1 - step : step;
        float acc[kSent];
#pragma unroll
        for (int s = 0; s < kSent; ++s) acc[s] = gn[s] + bj;
        if (step + 1 < T) {                                // the next step's G, in flight during this step's arithmetic
            const int tn = d ? t - 1 : t + 1;
#pragma unroll
            for (int s = 0; s < kSent; ++s) {
                const int b = b0 + s < B ? b0 + s : B - 1;
                gn[s] = gcol[((int64_t)b * T + tn) * ldg];
            }
        }
        // h.Whh^T: kHd / 4 x kSent / 4 pieces of four 16-byte broadcast reads and 16 FMAs; the reads of piece q + 1 are issued before
        // the FMAs of piece q and nothing moves across a piece (left alone, the scheduler gathers the reads and spills)
        float4 hv[4], hn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) hv[r] = *reinterpret_cast<const float4 *>(h_lds + r * kHd);
#pragma unroll
        for (int q = 0; q < kPieces; ++q) {
            const int k = (q / (kSent / 4)) * 4, s0 = (q % (kSent / 4)) * 4;
            if (q + 1 < kPieces) {
                const int kn = ((q + 1) / (kSent / 4)) * 4, sn = ((q + 1) % (kSent / 4)) * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) hn[r] = *reinterpret_cast<const float4 *>(h_lds + (sn + r) * kHd + kn);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float a = acc[s0 + r];
                a = fmaf(hv[r].x, w[k], a); a = fmaf(hv[r].y, w[k + 1], a);
                a = fmaf(hv[r].z, w[k + 2], a); a = fmaf(hv[r].w, w[k + 3], a);
                acc[s0 + r] = a;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 4; ++r) hv[r] = hn[r];
        }
        if (is_tanh) {
#pragma unroll
            for (int s = 0; s < kSent; ++s) act[s * kCols + j] = tanhf(acc[s]);
        } else {
#pragma unroll
            for (int s = 0; s < kSent; ++s) act[s * kCols + j] = sigmoidf(acc[s]);
        }
        if (SAVE) {   // the value just stored, over the element of G it was made from
#pragma unroll
            for (int s = 0; s < kSent; ++s)
                if (b0 + s < B) gates[((int64_t)(b0 + s) * T + t) * ldg + d * kCols + j] = act[s * kCols + j];
        }
        __syncthreads();   // the gates are in LDS; nobody reads h of the previous step any more
#pragma unroll
        for (int m = 0; m < kSent / 4; ++m) {
            const int s = sg + 4 * m;
            const float *a = act + s * kCols + u;
            if (SAVE && b0 + s < B) Hprev[((int64_t)(b0 + s) * T + t) * (2 * kHd) + d * kHd + u] = h_lds[s * kHd + u];
            c[m] = fmaf(a[kHd], c[m], a[0] * a[2 * kHd]);                  // c = f*c + i*g
            const float h = a[3 * kHd] * tanhf(c[m]);                      // h = o*tanh(c)
            h_lds[s * kHd + u] = h;
            if (b0 + s < B) Y[((int64_t)(b0 + s) * T + t) * ldy + d * kHd + u] = h;
            if (SAVE && b0 + s < B) C[((int64_t)(b0 + s) * T + t) * (2 * kHd) + d * kHd + u] = c[m];
        }
        __syncthreads();   // h of this step is in LDS; nobody reads this step's gates any more
    }
}

__global__ __launch_bounds__(kLstmThreads) void bilstm_recurrence_kernel(const float *__restrict__ G, int64_t ldg, const float *__restrict__ Whh_f,
                                                                         const float *__restrict__ Whh_r, const float *__restrict__ bias_f,
                                                                         const float *__restrict__ bias_r, float *__restrict__ Y, int64_t ldy,
                                                                         int B, int T)
{
    bilstm_recurrence_body<false>(G, ldg, Whh_f, Whh_r, bias_f, bias_r, Y, ldy, B, T, nullptr, nullptr, nullptr);
}

// (G and gates carry no __restrict__: they may be one buffer)
__global__ __launch_bounds__(kLstmThreads) void bilstm_recurrence_save_kernel(const float *G, int64_t ldg, const float *__restrict__ Whh_f,
                                                                              const float *__restrict__ Whh_r, const float *__restrict__ bias_f,
                                                                              const float *__restrict__ bias_r, float *__restrict__ Y, int64_t ldy,
                                                                              int B, int T, float *gates, float *__restrict__ C,
                                                                              float *__restrict__ Hprev)
{
    bilstm_recurrence_body<true>(G, ldg, Whh_f, Whh_r, bias_f, bias_r, Y, ldy, B, T, gates, C, Hprev);
}

// The backward of the recurrence.  Per sentence and direction, walking the direction's time backwards, with dh = dY + dh_rec and a
// carried dc:
//     tc = tanh(c_t)    do = dh*tc         dc += dh*o*(1-tc^2)
//     di = dc*g         dg = dc*i          df = dc*c_{t-1}          dc <- dc*f
//     da = [ di*i(1-i) | df*f(1-f) | dg*(1-g^2) | do*o(1-o) ]  -> dG          dh_rec = da . Whh_d
// Thread j is (u = j & 127, q = j >> 7) twice over: in the cell phase it owns the cells (s = q + 4 m, u), whose dc and dh_rec live
// in its registers, and writes their four da to LDS and to dG; in the product phase it owns output u of the quarter sum over the
// gate q's 128 rows, for the tile's 16 sentences.  A wavefront has one q, so every da read is one address for all its lanes.
__global__ __launch_bounds__(kLstmThreads) void bilstm_recurrence_backward_kernel(const float *__restrict__ dY, int64_t lddy,
                                                                                  const float *__restrict__ gates, int64_t ldg,
                                                                                  const float *__restrict__ C, const float *__restrict__ Whh_f,
                                                                                  const float *__restrict__ Whh_r, float *__restrict__ dG,
                                                                                  int64_t lddg, int B, int T)
{
    __shared__ __attribute__((aligned(16))) float da_lds[kSent * kCols];   // da of the tile's sentences at this step: [s][4hd]
    __shared__ float part[4 * kSent * kHd];                                 // the four quarter sums of dh_rec: [q][s][u]
    const int j = threadIdx.x, d = blockIdx.y, b0 = blockIdx.x * kSent;
    const int u = j & (kHd - 1), q = j >> 7;
    const float *__restrict__ whh = (d ? Whh_r : Whh_f) + (int64_t)q * kHd * kHd + u;
    float w[kHd];                                       // the column Whh_d[q*128 .. q*128+127, u]: coalesced across u
#pragma unroll
    for (int r = 0; r < kHd; ++r) w[r] = whh[r * kHd];
    constexpr int kCells = kSent / 4;
    float dc[kCells], dhr[kCells], cc[kCells];
    float ni[kCells], nf[kCells], ng[kCells], no[kCells], ny[kCells], np[kCells];   // the loads in flight: gates, dY, c_{t-1}
    // a sentence past B reads the batch's last sentence (its results are dropped)
    int64_t row0[kCells];
#pragma unroll
    for (int m = 0; m < kCells; ++m) {
        const int s = q + 4 * m, b = b0 + s < B ? b0 + s : B - 1;
        row0[m] = (int64_t)b * T;
        dc[m] = 0.0f;
        dhr[m] = 0.0f;
    }
    {
        const int t = d ? 0 : T - 1, tp = d ? t + 1 : t - 1;
#pragma unroll
        for (int m = 0; m < kCells; ++m) {
            const float *g = gates + (row0[m] + t) * ldg + d * kCols + u;
            ni[m] = g[0]; nf[m] = g[kHd]; ng[m] = g[2 * kHd]; no[m] = g[3 * kHd];
            ny[m] = dY[(row0[m] + t) * lddy + d * kHd + u];
            cc[m] = C[(row0[m] + t) * (2 * kHd) + d * kHd + u];
            np[m] = T > 1 ? C[(row0[m] + tp) * (2 * kHd) + d * kHd + u] : 0.0f;
        }
    }
    for (int step = 0; step < T; ++step) {
        const int t = d ? step : T - 1 - step;          // the step of the forward that is undone
        const int tn = d ? t + 1 : t - 1;               // the one undone next: the forward's previous step
        const bool more = step + 1 < T;
        float vi[kCells], vf[kCells], vg[kCells], vo[kCells], vy[kCells], vc[kCells], vp[kCells];
#pragma unroll
        for (int m = 0; m < kCells; ++m) {
            vi[m] = ni[m]; vf[m] = nf[m]; vg[m] = ng[m]; vo[m] = no[m]; vy[m] = ny[m]; vc[m] = cc[m]; vp[m] = np[m];
            cc[m] = vp[m];
        }
        if (more) {                                     // the next step's operands, in flight during this step's arithmetic
            const int tnn = d ? tn + 1 : tn - 1;
#pragma unroll
            for (int m = 0; m < kCells; ++m) {
                const float *g = gates + (row0[m] + tn) * ldg + d * kCols + u;
                ni[m] = g[0]; nf[m] = g[kHd]; ng[m] = g[2 * kHd]; no[m] = g[3 * kHd];
                ny[m] = dY[(row0[m] + tn) * lddy + d * kHd + u];
                np[m] = step + 2 < T ? C[(row0[m] + tnn) * (2 * kHd) + d * kHd + u] : 0.0f;   // (the direction's first step: c_{t-1} = 0)
            }
        }
#pragma unroll
        for (int m = 0; m < kCells; ++m) {
            const int s = q + 4 * m;
            const float dh = vy[m] + dhr[m];
            const float tc = tanhf(vc[m]);
            const float d_o = dh * tc;
            const float dcm = fmaf(dh * vo[m], 1.0f - tc * tc, dc[m]);
            const float di = dcm * vg[m], dg = dcm * vi[m], df = dcm * vp[m];
            dc[m] = dcm * vf[m];
            const float a0 = di * (vi[m] * (1.0f - vi[m])), a1 = df * (vf[m] * (1.0f - vf[m]));
            const float a2 = dg * (1.0f - vg[m] * vg[m]), a3 = d_o * (vo[m] * (1.0f - vo[m]));
            float *a = da_lds + s * kCols + u;
            a[0] = a0; a[kHd] = a1; a[2 * kHd] = a2; a[3 * kHd] = a3;
            if (b0 + s < B) {
                float *o = dG + (row0[m] + t) * lddg + d * kCols + u;
                o[0] = a0; o[kHd] = a1; o[2 * kHd] = a2; o[3 * kHd] = a3;
            }
        }
        if (!more) break;                               // (uniform) nothing reads the last step's dh_rec
        __syncthreads();   // da of this step is in LDS; nobody reads the previous step's quarter sums any more
        // da . Whh_d over the gate q's rows: the forward's pieces -- four 16-byte broadcast reads and 16 FMAs, the reads of piece
        // p + 1 issued before the FMAs of piece p, nothing moved across a piece
        float acc[kSent];
#pragma unroll
        for (int s = 0; s < kSent; ++s) acc[s] = 0.0f;
        const float *dq = da_lds + q * kHd;
        float4 hv[4], hn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) hv[r] = *reinterpret_cast<const float4 *>(dq + r * kCols);
#pragma unroll
        for (int p = 0; p < kPieces; ++p) {
            const int k = (p / (kSent / 4)) * 4, s0 = (p % (kSent / 4)) * 4;
            if (p + 1 < kPieces) {
                const int kn = ((p + 1) / (kSent / 4)) * 4, sn = ((p + 1) % (kSent / 4)) * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) hn[r] = *reinterpret_cast<const float4 *>(dq + (sn + r) * kCols + kn);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float a = acc[s0 + r];
                a = fmaf(hv[r].x, w[k], a); a = fmaf(hv[r].y, w[k + 1], a);
                a = fmaf(hv[r].z, w[k + 2], a); a = fmaf(hv[r].w, w[k + 3], a);
                acc[s0 + r] = a;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 4; ++r) hv[r] = hn[r];
        }
#pragma unroll
        for (int s = 0; s < kSent; ++s) part[(q * kSent + s) * kHd + u] = acc[s];
        __syncthreads();   // the quarter sums are in LDS; nobody reads this step's da any more
#pragma unroll
        for (int m = 0; m < kCells; ++m) {
            const float *pq = part + (q + 4 * m) * kHd + u;
            dhr[m] = ((pq[0] + pq[kSent * kHd]) + pq[2 * kSent * kHd]) + pq[3 * kSent * kHd];   // q = 0, 1, 2, 3
        }
    }
}

// the refusals the three entries share, in the order of ggcn_bilstm_recurrence's
int recurrence_checks(const char *who, bool null, int B, int T, int hd, bool ld_ok, const float *Whh_f, const float *Whh_r)
{
    if (null) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (B <= 0 || T <= 0) return fail(GGCN_EINVAL, "%s: B=%d T=%d must be positive", who, B, T);
    if (hd != kHd) return fail(GGCN_EUNSUPPORTED, "%s: hd=%d (the kernel is built for hd = 128, bert_amir5.py:551)", who, hd);
    if (!ld_ok) return fail(GGCN_EINVAL, "%s: leading dimension too small", who);
    if ((int64_t)B * T >= ((int64_t)1 << 31)) return fail(GGCN_EUNSUPPORTED, "%s: B*T=%lld rows (at most 2^31 - 1)", who, (long long)B * T);
    if (!aligned16(Whh_f) || !aligned16(Whh_r)) return fail(GGCN_EINVAL, "%s: Whh_f and Whh_r must be 16-byte aligned", who);
    return GGCN_OK;
}

}  // namespace
}  // namespace ggcn

extern "C" int ggcn_bilstm_recurrence_save(const float *G, int64_t ldg, const float *Whh_f, const float *Whh_r, const float *bias_f,
                                           const float *bias_r, float *Y, int64_t ldy, int B, int T, int hd, float *gates, float *C,
                                           float *Hprev, ggcn_stream_t stream)
{
    using namespace ggcn;
    const char *who = "ggcn_bilstm_recurrence_save";
    if (int rc = recurrence_checks(who, !G || !Whh_f || !Whh_r || !Y || !gates || !C || !Hprev, B, T, hd,
                                   ldg >= 8 * (int64_t)hd && ldy >= 2 * (int64_t)hd, Whh_f, Whh_r))
        return rc;
    hipLaunchKernelGGL(bilstm_recurrence_save_kernel, dim3((unsigned)((B + kSent - 1) / kSent), 2u), dim3(kLstmThreads), 0, as_stream(stream), G,
                       ldg, Whh_f, Whh_r, bias_f, bias_r, Y, ldy, B, T, gates, C, Hprev);
    return check_launch(who);
}

extern "C" int ggcn_bilstm_recurrence_backward(const float *dY, int64_t lddy, const float *gates, int64_t ldg, const float *C,
                                               const float *Whh_f, const float *Whh_r, float *dG, int64_t lddg, int B, int T, int hd,
                                               ggcn_stream_t stream)
{
    using namespace ggcn;
    const char *who = "ggcn_bilstm_recurrence_backward";
    if (int rc = recurrence_checks(who, !dY || !gates || !C || !Whh_f || !Whh_r || !dG, B, T, hd,
                                   lddy >= 2 * (int64_t)hd && ldg >= 8 * (int64_t)hd && lddg >= 8 * (int64_t)hd, Whh_f, Whh_r))
        return rc;
    {   // dG is a buffer of its own: a second backward (retain_graph) reads the gates again
        const int64_t rows = (int64_t)B * T;
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(gates), d0 = reinterpret_cast<uintptr_t>(dG);
        const uintptr_t g1 = g0 + (uintptr_t)((rows - 1) * ldg + 8 * hd) * sizeof(float), d1 = d0 + (uintptr_t)((rows - 1) * lddg + 8 * hd) * sizeof(float);
        if (d0 < g1 && g0 < d1) return fail(GGCN_EINVAL, "%s: dG must not alias gates", who);
    }
    hipLaunchKernelGGL(bilstm_recurrence_backward_kernel, dim3((unsigned)((B + kSent - 1) / kSent), 2u), dim3(kLstmThreads), 0, as_stream(stream),
                       dY, lddy, gates, ldg, C, Whh_f, Whh_r, dG, lddg, B, T);
    return check_launch(who);
}

extern "C" int ggcn_bilstm_recurrence(const float *G, int64_t ldg, const float *Whh_f, const float *Whh_r, const float *bias_f,
                                      const float *bias_r, float *Y, int64_t ldy, int B, int T, int hd, ggcn_stream_t stream)
{
    using namespace ggcn;
    const char *who = "ggcn_bilstm_recurrence";
    if (int rc = recurrence_checks(who, !G || !Whh_f || !Whh_r || !Y, B, T, hd, ldg >= 8 * (int64_t)hd && ldy >= 2 * (int64_t)hd, Whh_f, Whh_r))
        return rc;
    hipLaunchKernelGGL(bilstm_recurrence_kernel, dim3((unsigned)((B + kSent - 1) / kSent), 2u), dim3(kLstmThreads), 0, as_stream(stream), G, ldg,
                       Whh_f, Whh_r, bias_f, bias_r, Y, ldy, B, T);
    return check_launch(who);
}
