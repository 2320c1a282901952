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
#include "common.h"

namespace ggcn {
namespace {

constexpr int kHd = 128, kCols = 4 * kHd, kSent = GGCN_BILSTM_TILE, kLstmThreads = kCols;
constexpr int kPieces = (kHd / 4) * (kSent / 4);
static_assert(kSent % 4 == 0, "four cell groups share a tile's sentences");

// 0 / 1 for |v| ~ 1e4 without a NaN: expf(-v) overflows to +inf on the negative side (1 / inf = 0) and is 0 on the positive one
__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ __launch_bounds__(kLstmThreads) void bilstm_recurrence_kernel(const float *__restrict__ G, int64_t ldg, const float *__restrict__ Whh_f,
                                                                         const float *__restrict__ Whh_r, const float *__restrict__ bias_f,
                                                                         const float *__restrict__ bias_r, float *__restrict__ Y, int64_t ldy,
                                                                         int B, int T)
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
        __syncthreads();   // the gates are in LDS; nobody reads h of the previous step any more
#pragma unroll
        for (int m = 0; m < kSent / 4; ++m) {
            const int s = sg + 4 * m;
            const float *a = act + s * kCols + u;
            c[m] = fmaf(a[kHd], c[m], a[0] * a[2 * kHd]);                  // c = f*c + i*g
            const float h = a[3 * kHd] * tanhf(c[m]);                      // h = o*tanh(c)
            h_lds[s * kHd + u] = h;
            if (b0 + s < B) Y[((int64_t)(b0 + s) * T + t) * ldy + d * kHd + u] = h;
        }
        __syncthreads();   // h of this step is in LDS; nobody reads this step's gates any more
    }
}

}  // namespace
}  // namespace ggcn

extern "C" int ggcn_bilstm_recurrence(const float *G, int64_t ldg, const float *Whh_f, const float *Whh_r, const float *bias_f,
                                      const float *bias_r, float *Y, int64_t ldy, int B, int T, int hd, ggcn_stream_t stream)
{
    using namespace ggcn;
    const char *who = "ggcn_bilstm_recurrence";
    if (!G || !Whh_f || !Whh_r || !Y) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (B <= 0 || T <= 0) return fail(GGCN_EINVAL, "%s: B=%d T=%d must be positive", who, B, T);
    if (hd != kHd) return fail(GGCN_EUNSUPPORTED, "%s: hd=%d (the kernel is built for hd = 128, bert_amir5.py:551)", who, hd);
    if (ldg < 8 * (int64_t)hd || ldy < 2 * (int64_t)hd) return fail(GGCN_EINVAL, "%s: leading dimension too small", who);
    if ((int64_t)B * T >= ((int64_t)1 << 31)) return fail(GGCN_EUNSUPPORTED, "%s: B*T=%lld rows (at most 2^31 - 1)", who, (long long)B * T);
    if (!aligned16(Whh_f) || !aligned16(Whh_r)) return fail(GGCN_EINVAL, "%s: Whh_f and Whh_r must be 16-byte aligned", who);
    hipLaunchKernelGGL(bilstm_recurrence_kernel, dim3((unsigned)((B + kSent - 1) / kSent), 2u), dim3(kLstmThreads), 0, as_stream(stream), G, ldg,
                       Whh_f, Whh_r, bias_f, bias_r, Y, ldy, B, T);
    return check_launch(who);
}
