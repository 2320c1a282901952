// The two small pieces of BertAmir55.forward that sit directly on either side of the gated block
// (SURVEY 8f ranks 1 and 4), each as ONE launch:
//
//   gate MLPs    models/bert_amir5.py:562-571,621-622   gate_k = Sigmoid(Linear(Sigmoid(Linear(Sigmoid(aspect)))))
//                for k = 1, 2: [B,H] -> two [B,H] gates (the reference then repeats them to [B,T,H]; here they
//                stay [B,H] and go straight into ggcn_block_fused / ggcn_layer_fused)
//   scores / kl  models/bert_amir5.py:645-648           output_w = fc(cat[x, aspect]); scores = sum_c logits*output_w;
//                kl = mean_b sum_t softmax_t(scores) * softmax_t(dist)
//
// scores needs no [B,T,C] intermediate: fc(cat[x_t, a]) = Wx.x_t + Wa.a + b, so
//     scores[b,t] = logits_b . (Wx.x_t + Wa.a_b + b) = (Wx^T.logits_b) . x_t + logits_b . (Wa.a_b + b)
// -- one H-vector and one scalar per sentence, then one dot product per token: x is read once (HBM-bound).
// Both kernels use plain fp32 FMA chains (exact fp32, no matrix cores: 0.1-0.3 GFLOP at the reference's
// batch of 256 sentences).  The scores / kl head also has its backward here, for training through it: one launch per call
// (scores_head_backward_kernel) and a fixed-order weight product (head_dweight_*_kernel).  So have the gate MLPs: the forward
// in a form that keeps the hidden activations (gate_mlp_kernel<true>) and one backward launch (gate_mlp_backward_kernel) that
// leaves the operands of the library's own weight products.
#include "common.h"

namespace ggcn {
namespace {

__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

// Wt[k][j] = W[j][k] for an nn.Linear weight W [out, in] (contiguous): once per weight update
__global__ __launch_bounds__(256) void transpose_kernel(const float *__restrict__ W, int rows, int cols, int64_t ldw,
                                                        float *__restrict__ Wt)
{
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = W[(int64_t)(r0 + i) * ldw + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < cols && r0 + tx < rows) Wt[(int64_t)(c0 + i) * rows + r0 + tx] = tile[tx][i];
}

struct GateParams {
    const float *w1t, *b1, *w2t, *b2;   // transposed weights [in=H][out=H], biases [H]
    float *out;                         // [B,H]
    float *hid;                         // [B,H]: the hidden sigmoid, kept for the backward (SAVE form only)
};

constexpr int kGateRows = 8;   // sentences per workgroup

// grid (ceil(B / 8), 2 gates); dynamic LDS: 2 * 8 * H floats.  SAVE (ggcn_gate_mlp_save, the forward under autograd): the
// hidden activations h also go to memory; the gates are the bits of the plain form.
template <bool SAVE>
__global__ __launch_bounds__(256) void gate_mlp_kernel(const float *__restrict__ aspect, int64_t lda, int B, int H,
                                                       GateParams ga, GateParams gb)
{
    extern __shared__ float lds_f[];
    float *s = lds_f, *h = lds_f + kGateRows * H;
    const GateParams gp = blockIdx.y == 0 ? ga : gb;
    const int r0 = blockIdx.x * kGateRows;
    const int nr = B - r0 < kGateRows ? B - r0 : kGateRows;
    for (int i = threadIdx.x; i < kGateRows * H; i += 256) {
        const int r = i / H, k = i - r * H;
        s[i] = r < nr ? sigmoidf(aspect[(int64_t)(r0 + r) * lda + k]) : 0.0f;       // the Sequential's leading Sigmoid
    }
    __syncthreads();
    for (int layer = 0; layer < 2; ++layer) {
        const float *wt = layer == 0 ? gp.w1t : gp.w2t, *bias = layer == 0 ? gp.b1 : gp.b2;
        const float *in = layer == 0 ? s : h;
        for (int j = threadIdx.x; j < H; j += 256) {
            float acc[kGateRows];
#pragma unroll
            for (int r = 0; r < kGateRows; ++r) acc[r] = 0.0f;
            for (int k = 0; k < H; ++k) {
                const float w = wt[(int64_t)k * H + j];        // lanes = consecutive j: one coalesced row piece per k
#pragma unroll
                for (int r = 0; r < kGateRows; ++r) acc[r] = fmaf(in[r * H + k], w, acc[r]);
            }
            const float bj = bias ? bias[j] : 0.0f;
            if (layer == 0) {
#pragma unroll
                for (int r = 0; r < kGateRows; ++r) {
                    const float hv = sigmoidf(acc[r] + bj);
                    h[r * H + j] = hv;
                    if (SAVE && r < nr) gp.hid[(int64_t)(r0 + r) * H + j] = hv;
                }
            } else {
#pragma unroll
                for (int r = 0; r < kGateRows; ++r)
                    if (r < nr) gp.out[(int64_t)(r0 + r) * H + j] = sigmoidf(acc[r] + bj);
            }
        }
        __syncthreads();
    }
}

// ---- backward of the gate MLPs (training through bert_amir5.py:562-571) ----------------------------------------------------
// Per gate, with s = sigmoid(a), h = sigmoid(s.W1^T + b1), g = sigmoid(h.W2^T + b2) and the incoming dG [B,H]:
//     dz2 = dG * g(1-g)      dh = dz2.W2      dz1 = dh * h(1-h)      ds = dz1.W1      da = (ds_A + ds_B) * s(1-s)
// h and g are the forward's stored float32 values (ggcn_gate_mlp_save); s is recomputed.  W1, W2 are read in nn.Linear's own
// [out][in] layout: the products run over the rows j of W, so a thread that owns column k reads one coalesced row piece per j.
// One workgroup per 8 sentences, gate A and then gate B, like the forward; two 8 x H LDS buffers (dz2, then dz1), 8
// accumulators per column and all of a thread's columns k = tid, tid + 256, ... in one walk over j (each LDS read serves
// them all), exact fp32 FMA chains with j ascending.  After gate A a thread stores its ds element into d_aspect;
// after gate B the same thread reads that element again, adds to it and applies s(1-s): no atomics, the same bits on every
// call.  Z [B, ldz] receives what the weight products read: dz1_A | dz1_B | dz2_A | dz2_B | s, each group Hp = H rounded up
// to 4 columns wide (the up to 3 columns behind a group's H are written as zeros); a gate without an incoming gradient
// contributes nothing to d_aspect and its groups are zeros.
struct GateGrad {
    const float *w1, *w2;             // nn.Linear weights [out=H][in=H], contiguous
    const float *hid, *gate, *dg;     // [B,H] contiguous; dg NULL: no gradient reached this gate
};

// acc[c][r] += sum_j in[r][j] * W[j][k_c], j ascending, for the thread's NC columns k_c = tid + 256 c at once: one LDS
// broadcast read of in[r][j] serves all of them (a column past H reads column 0 and is dropped by the caller).
// VEC: H % 4 == 0, four j per step through one 16-byte LDS read per row; the order of every sum is the scalar loop's.
template <bool VEC, int NC>
__device__ __forceinline__ void gate_rows_times_columns(const float *in, const float *__restrict__ W, int H, int tid,
                                                        float (&acc)[NC][kGateRows])
{
    int kc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        kc[c] = tid + 256 * c < H ? tid + 256 * c : 0;
#pragma unroll
        for (int r = 0; r < kGateRows; ++r) acc[c][r] = 0.0f;
    }
    if (VEC) {
        for (int j = 0; j < H; j += 4) {
            float w[NC][4];
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[c][q] = W[(int64_t)(j + q) * H + kc[c]];
#pragma unroll
            for (int r = 0; r < kGateRows; ++r) {
                const float4 v = *reinterpret_cast<const float4 *>(in + r * H + j);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    acc[c][r] = fmaf(v.x, w[c][0], acc[c][r]); acc[c][r] = fmaf(v.y, w[c][1], acc[c][r]);
                    acc[c][r] = fmaf(v.z, w[c][2], acc[c][r]); acc[c][r] = fmaf(v.w, w[c][3], acc[c][r]);
                }
            }
        }
    } else {
#pragma unroll 2
        for (int j = 0; j < H; ++j) {
            float w[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) w[c] = W[(int64_t)j * H + kc[c]];
#pragma unroll
            for (int r = 0; r < kGateRows; ++r) {
                const float v = in[r * H + j];
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c][r] = fmaf(v, w[c], acc[c][r]);
            }
        }
    }
}

// grid ceil(B / 8); dynamic LDS: 2 * 8 * H floats; NC = ceil(H / 256) columns per thread (H <= 1024: at most 4)
template <bool VEC, int NC>
__global__ __launch_bounds__(256) void gate_mlp_backward_kernel(const float *__restrict__ aspect, int64_t lda, int B, int H, GateGrad ga,
                                                                GateGrad gb, float *d_aspect, int64_t ldda, float *__restrict__ Z,
                                                                int64_t ldz)
{
    extern __shared__ __attribute__((aligned(16))) float gate_bwd_lds[];
    float *dz2 = gate_bwd_lds, *dz1 = gate_bwd_lds + kGateRows * H;
    const int tid = threadIdx.x, Hp = (H + 3) & ~3;
    const int r0 = blockIdx.x * kGateRows;
    const int nr = B - r0 < kGateRows ? B - r0 : kGateRows;
    if (Z) {
        for (int i = tid; i < nr * H; i += 256) {                  // the s group: the other operand of dW1 = dz1^T.s
            const int r = i / H, k = i - r * H;
            Z[(int64_t)(r0 + r) * ldz + 4 * Hp + k] = sigmoidf(aspect[(int64_t)(r0 + r) * lda + k]);
        }
        const int pad = Hp - H;                                    // 0..3 columns behind each of the five groups
        for (int i = tid; i < nr * 5 * pad; i += 256) {
            const int r = i / (5 * pad), q = i - r * 5 * pad, g = q / pad;
            Z[(int64_t)(r0 + r) * ldz + g * Hp + H + (q - g * pad)] = 0.0f;
        }
    }
    const bool both = ga.dg && gb.dg;
    for (int gi = 0; gi < 2; ++gi) {
        const GateGrad gp = gi == 0 ? ga : gb;
        float *z1 = Z ? Z + gi * Hp : nullptr, *z2 = Z ? Z + (2 + gi) * Hp : nullptr;
        if (!gp.dg) {                                              // (kernel-uniform)
            if (Z)
                for (int i = tid; i < nr * H; i += 256) {
                    const int r = i / H, k = i - r * H;
                    z1[(int64_t)(r0 + r) * ldz + k] = 0.0f;
                    z2[(int64_t)(r0 + r) * ldz + k] = 0.0f;
                }
            continue;
        }
        for (int i = tid; i < kGateRows * H; i += 256) {           // dz2 = dG * g(1-g)
            const int r = i / H, k = i - r * H;
            float v = 0.0f;
            if (r < nr) {
                const int64_t at = (int64_t)(r0 + r) * H + k;
                const float g = gp.gate[at];
                v = gp.dg[at] * (g * (1.0f - g));
                if (z2) z2[(int64_t)(r0 + r) * ldz + k] = v;
            }
            dz2[i] = v;
        }
        __syncthreads();
        float acc[NC][kGateRows];
        gate_rows_times_columns<VEC, NC>(dz2, gp.w2, H, tid, acc);       // dz1 = (dz2.W2) * h(1-h)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int k = tid + 256 * c;
            if (k >= H) continue;
#pragma unroll
            for (int r = 0; r < kGateRows; ++r) {
                float v = 0.0f;
                if (r < nr) {
                    const float h = gp.hid[(int64_t)(r0 + r) * H + k];
                    v = acc[c][r] * (h * (1.0f - h));
                    if (z1) z1[(int64_t)(r0 + r) * ldz + k] = v;
                }
                dz1[r * H + k] = v;
            }
        }
        __syncthreads();   // (also: nobody still reads dz2 when the next gate overwrites it, nor dz1 one barrier later)
        if (!d_aspect) continue;
        gate_rows_times_columns<VEC, NC>(dz1, gp.w1, H, tid, acc);       // ds = dz1.W1; d a = (ds_A + ds_B) * s(1-s)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int k = tid + 256 * c;
            if (k >= H) continue;
#pragma unroll
            for (int r = 0; r < kGateRows; ++r) {
                if (r >= nr) continue;
                float *p = d_aspect + (int64_t)(r0 + r) * ldda + k;
                if (both && gi == 0) {
                    *p = acc[c][r];                                // gate A's share, picked up again by this thread after gate B
                } else {
                    const float ds = both ? *p + acc[c][r] : acc[c][r];
                    const float s = sigmoidf(aspect[(int64_t)(r0 + r) * lda + k]);
                    *p = ds * (s * (1.0f - s));
                }
            }
        }
    }
}

// one workgroup per sentence; dynamic LDS: (H + C + T + 8) floats
__global__ __launch_bounds__(256) void scores_head_kernel(const float *__restrict__ X, int64_t ldx,
                                                          const float *__restrict__ aspect, int64_t lda,
                                                          const float *__restrict__ logits, int64_t ldl,
                                                          const float *__restrict__ fcw, int64_t ldw,
                                                          const float *__restrict__ fcb, const float *__restrict__ dist,
                                                          int64_t ldd, int T, int H, int C, float *__restrict__ scores,
                                                          int64_t lds_, float *__restrict__ kl_part)
{
    extern __shared__ float lds_f[];
    float *v = lds_f, *u = v + H, *sc = u + C, *red = sc + T;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *lg = logits + (int64_t)b * ldl, *a = aspect + (int64_t)b * lda;
    // v[h] = sum_c logits[c] * Wx[c][h]  (Wx = the first H columns of fc.weight [C, 2H])
    for (int hh = tid; hh < H; hh += 256) {
        float acc = 0.0f;
        for (int c = 0; c < C; ++c) acc = fmaf(lg[c], fcw[(int64_t)c * ldw + hh], acc);
        v[hh] = acc;
    }
    // u[c] = Wa[c,:] . a + b[c]   (wavefront per class, lanes over h)
    for (int c = wave; c < C; c += 4) {
        float acc = 0.0f;
        for (int hh = lane; hh < H; hh += 64) acc = fmaf(fcw[(int64_t)c * ldw + H + hh], a[hh], acc);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) u[c] = acc + (fcb ? fcb[c] : 0.0f);
    }
    __syncthreads();
    float c0 = 0.0f;
    for (int c = 0; c < C; ++c) c0 = fmaf(lg[c], u[c], c0);       // the same fixed order in every thread
    // scores[t] = v . x_t + c0   (wavefront per token, lanes over h: coalesced row reads)
    for (int t = wave; t < T; t += 4) {
        const float *xr = X + ((int64_t)b * T + t) * ldx;
        float acc = 0.0f;
        for (int hh = lane; hh < H; hh += 64) acc = fmaf(xr[hh], v[hh], acc);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) {
            sc[t] = acc + c0;
            scores[(int64_t)b * lds_ + t] = acc + c0;
        }
    }
    __syncthreads();
    if (!kl_part) return;
    // kl_b = sum_t softmax_t(scores) * softmax_t(dist): one wavefront, fixed order
    if (wave == 0) {
        const float *dr = dist + (int64_t)b * ldd;
        float ms = -INFINITY, md = -INFINITY;
        for (int t = lane; t < T; t += 64) { ms = fmaxf(ms, sc[t]); md = fmaxf(md, dr[t]); }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { ms = fmaxf(ms, __shfl_xor(ms, d)); md = fmaxf(md, __shfl_xor(md, d)); }
        float zs = 0.0f, zd = 0.0f, cross = 0.0f;
        for (int t = lane; t < T; t += 64) {
            const float es = expf(sc[t] - ms), ed = expf(dr[t] - md);
            zs += es; zd += ed; cross = fmaf(es, ed, cross);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { zs += __shfl_xor(zs, d); zd += __shfl_xor(zd, d); cross += __shfl_xor(cross, d); }
        if (lane == 0) kl_part[b] = cross / (zs * zd);
    }
    (void)red;
}

// ---- backward of the scores / kl head (training through bert_amir5.py:645-648) -------------------------------------------
// With v = Wx^T.lg, u = Wa.a + fb, c0 = lg.u, scores[t] = v.x_t + c0, p = softmax_t(scores), q = softmax_t(dist),
// kl_b = sum_t p_t q_t and the incoming g_s [B,T] (d scores) and g_k (d kl, one device float), per sentence:
//     ds[t]  = g_s[t] + (g_k / B) p_t (q_t - kl_b)
//     dX[t]  = ds[t] v            dv = sum_t ds[t] x_t          dc0 = sum_t g_s[t]
//     d lg   = Wx.dv + dc0 u      d a = dc0 (Wa^T.lg)           G = [dv | dc0 a]   (dW = lg^T.G and dfb = lg^T.dc0: below)
// dc0 is the sum of ds over t; the kl term's share of that sum is sum_t p_t (q_t - kl_b) = 0 identically (a softmax does not
// see a shift of its scores), so it is left out instead of being summed to rounding noise: a loss that uses kl alone gives
// exact zeros for d a, dWa and dfb, as the mathematics does.
// One workgroup per sentence, like the forward.  v, u and the two softmaxes are recomputed (the forward's own loops, on the
// saved scores and kl_b); then ONE pass over the sentence's x rows: wavefront w takes the tokens t = w, w + 4, ..., lanes over
// h; per 256-column (scalar form: 64-column) chunk a lane keeps its piece of v and of the wavefront's dv in registers, reads
// x[t] once, stores dX[t] once.  The four wavefronts' dv meet in LDS in the order 0, 1, 2, 3.  Every sum has a fixed order
// (t ascending per wavefront, xor butterflies, wavefronts ascending): no atomics, the same bits on every call.
// Dynamic LDS: v [Hp] | dv of the 4 wavefronts [4][Hp] | Wa^T.lg [Hp] | u [C] | ds [T] | 8 floats, Hp = H rounded up to 4 (16-byte carves).
// sum_c lg[c] * W[c][col], c ascending (one FMA chain, as the forward's v), the loads of eight classes in flight at a time
__device__ __forceinline__ float column_dot(const float *__restrict__ lg, const float *__restrict__ wcol, int64_t ldw, int C)
{
    float acc = 0.0f;
    int c = 0;
    for (; c + 8 <= C; c += 8) {
        float w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = wcol[(int64_t)(c + q) * ldw];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = fmaf(lg[c + q], w[q], acc);
    }
    for (; c < C; ++c) acc = fmaf(lg[c], wcol[(int64_t)c * ldw], acc);
    return acc;
}

template <bool VEC>
__global__ __launch_bounds__(256) void scores_head_backward_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ aspect, int64_t lda, const float *__restrict__ logits,
    int64_t ldl, const float *__restrict__ fcw, int64_t ldw, const float *__restrict__ fcb, const float *__restrict__ dist,
    int64_t ldd, const float *__restrict__ scores, int64_t lds_, const float *__restrict__ kl_part,
    const float *__restrict__ g_scores, int64_t ldgs, const float *__restrict__ g_kl, int B, int T, int H, int C,
    float *__restrict__ dX, int64_t lddx, float *__restrict__ d_aspect, int64_t ldda, float *__restrict__ d_logits, int64_t lddl,
    float *__restrict__ G, int64_t ldg, float *__restrict__ dc0_out)
{
    extern __shared__ __attribute__((aligned(16))) float bwd_lds[];
    const int Hp = (H + 3) & ~3;
    float *v = bwd_lds, *dvp = v + Hp, *wal = dvp + 4 * Hp, *u = wal + Hp, *ds = u + C, *red = ds + T;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *lg = logits + (int64_t)b * ldl, *a = aspect + (int64_t)b * lda;
    // v = Wx^T.lg (the forward's sums, class by class) and, for d a, Wa^T.lg: one loop over fc.weight's 2H columns
    for (int col = tid; col < (d_aspect ? 2 * H : H); col += 256) {
        const float s = column_dot(lg, fcw + col, ldw, C);
        if (col < H) v[col] = s;
        else wal[col - H] = s;
    }
    for (int c = wave; c < C; c += 4) {                           // u: the forward's loop
        float acc = 0.0f;
#pragma unroll 4
        for (int hh = lane; hh < H; hh += 64) acc = fmaf(fcw[(int64_t)c * ldw + H + hh], a[hh], acc);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) u[c] = acc + (fcb ? fcb[c] : 0.0f);
    }
    if (wave == 0) {                                              // ds [T] and dc0: one wavefront, lanes loop over t
        const float *gs = g_scores ? g_scores + (int64_t)b * ldgs : nullptr;
        float sum_gs = 0.0f;
        for (int t = lane; t < T; t += 64) {
            const float g = gs ? gs[t] : 0.0f;
            ds[t] = g;
            sum_gs += g;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum_gs += __shfl_xor(sum_gs, d);
        if (lane == 0) red[0] = sum_gs;
        if (g_kl) {
            const float *sr = scores + (int64_t)b * lds_, *dr = dist + (int64_t)b * ldd;
            float ms = -INFINITY, md = -INFINITY;
            for (int t = lane; t < T; t += 64) { ms = fmaxf(ms, sr[t]); md = fmaxf(md, dr[t]); }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { ms = fmaxf(ms, __shfl_xor(ms, d)); md = fmaxf(md, __shfl_xor(md, d)); }
            float zs = 0.0f, zd = 0.0f;
            for (int t = lane; t < T; t += 64) { zs += expf(sr[t] - ms); zd += expf(dr[t] - md); }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { zs += __shfl_xor(zs, d); zd += __shfl_xor(zd, d); }
            const float gk = *g_kl / (float)B, klb = kl_part[b];
            for (int t = lane; t < T; t += 64)                     // (each lane re-reads the ds[t] it wrote itself)
                ds[t] = fmaf(gk * (expf(sr[t] - ms) / zs), expf(dr[t] - md) / zd - klb, ds[t]);
        }
    }
    __syncthreads();
    const float dc0 = red[0];
    const int64_t row0 = (int64_t)b * T;
    if (VEC) {      // H % 4 == 0, 16-byte-aligned rows of X and dX: a lane takes 4 columns of every 256
        for (int h0 = 4 * lane; h0 < H; h0 += 256) {
            const float4 vv = *reinterpret_cast<const float4 *>(v + h0);
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
            for (int t = wave; t < T; t += 4) {
                const float d = ds[t];
                const float4 xv = *reinterpret_cast<const float4 *>(X + (row0 + t) * ldx + h0);
                acc.x = fmaf(d, xv.x, acc.x); acc.y = fmaf(d, xv.y, acc.y);
                acc.z = fmaf(d, xv.z, acc.z); acc.w = fmaf(d, xv.w, acc.w);
                if (dX) *reinterpret_cast<float4 *>(dX + (row0 + t) * lddx + h0) = make_float4(d * vv.x, d * vv.y, d * vv.z, d * vv.w);
            }
            *reinterpret_cast<float4 *>(dvp + wave * Hp + h0) = acc;
        }
    } else {        // any H, any alignment: a lane takes 1 column of every 64
        for (int hh = lane; hh < H; hh += 64) {
            const float vh = v[hh];
            float acc = 0.0f;
#pragma unroll 4
            for (int t = wave; t < T; t += 4) {
                const float d = ds[t];
                acc = fmaf(d, X[(row0 + t) * ldx + hh], acc);
                if (dX) dX[(row0 + t) * lddx + hh] = d * vh;
            }
            dvp[wave * Hp + hh] = acc;
        }
    }
    __syncthreads();
    for (int hh = tid; hh < H; hh += 256) {
        const float dv = ((dvp[hh] + dvp[Hp + hh]) + dvp[2 * Hp + hh]) + dvp[3 * Hp + hh];   // wavefronts 0, 1, 2, 3
        dvp[hh] = dv;                                              // (this thread's own column: read again after the barrier)
        if (G) {
            G[(int64_t)b * ldg + hh] = dv;
            G[(int64_t)b * ldg + H + hh] = dc0 * a[hh];
        }
        if (d_aspect) d_aspect[(int64_t)b * ldda + hh] = dc0 * wal[hh];   // d a = dc0 * (Wa^T . lg)
    }
    __syncthreads();
    if (d_logits)
        for (int c = wave; c < C; c += 4) {                        // d lg[c] = Wx[c,:] . dv + dc0 u[c]: u's loop on the first half
            float acc = 0.0f;
#pragma unroll 4
            for (int hh = lane; hh < H; hh += 64) acc = fmaf(fcw[(int64_t)c * ldw + hh], dvp[hh], acc);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
            if (lane == 0) d_logits[(int64_t)b * lddl + c] = fmaf(dc0, u[c], acc);
        }
    if (dc0_out && tid == 0) dc0_out[b] = dc0;
}

// dW = lg^T . G  ([C,B] x [B,2H]) and dfb = lg^T . dc0 of the head, in a fixed order: G's columns and dc0 as column 2H; the
// launch's z slices take kDwRows sentences each (b ascending) into part [slices][C][2H + 1], a second launch adds the slices in
// ascending order.  0.4 GFLOP at 4096 x 768 x 34: exact fp32 FMA chains, lg read through scalar loads (uniform per workgroup).
constexpr int kDwRows = 128, kDwClasses = 8;
__global__ __launch_bounds__(256) void head_dweight_partial_kernel(const float *__restrict__ logits, int64_t ldl, const float *__restrict__ G,
                                                                   int64_t ldg, const float *__restrict__ dc0, int B, int W2, int C,
                                                                   float *__restrict__ part)
{
    const int j = blockIdx.x * 256 + threadIdx.x, c0 = blockIdx.y * kDwClasses, b0 = blockIdx.z * kDwRows;
    const int b1 = b0 + kDwRows < B ? b0 + kDwRows : B;
    if (j > W2) return;
    float acc[kDwClasses] = {};
    for (int b = b0; b < b1; ++b) {
        const float g = j < W2 ? G[(int64_t)b * ldg + j] : dc0[b];
#pragma unroll
        for (int q = 0; q < kDwClasses; ++q) acc[q] = fmaf(c0 + q < C ? logits[(int64_t)b * ldl + c0 + q] : 0.0f, g, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < kDwClasses; ++q)
        if (c0 + q < C) part[((int64_t)blockIdx.z * C + c0 + q) * (W2 + 1) + j] = acc[q];
}

__global__ __launch_bounds__(256) void head_dweight_finish_kernel(const float *__restrict__ part, int slices, int W2, int C, float *__restrict__ dW,
                                                                  int64_t lddw, float *__restrict__ dfb)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, n = (int64_t)C * (W2 + 1);
    if (idx >= n) return;
    const int c = (int)(idx / (W2 + 1)), j = (int)(idx - (int64_t)c * (W2 + 1));
    float t = 0.0f;
    for (int s = 0; s < slices; ++s) t += part[(int64_t)s * n + idx];
    if (j < W2) dW[(int64_t)c * lddw + j] = t;
    else if (dfb) dfb[c] = t;
}


// ---- dense head on the pooled output (bert_amir5.py:643: the share of `dense` that reads the block's `out`) ------------
// logits[b,c] = bias[c] + sum_k pooled[b,k] * Wt[k,c], C <= 64.  One workgroup of 16 wavefronts per 8 sentences: their pooled
// rows go to LDS, lane = class, wavefront w takes k-slice w (Wt rows are read coalesced and all at once), the slices
// meet in LDS in a fixed order: a row's logits do not depend on which batch (or shard) the row sits in.  The LAST workgroup
// of the launch, when the caller passes them, adds the regulariser's partials of a ggcn_block_fused launch (bert_amir5.py:638)
// in a fixed order of its own (a 1024-thread stride, a wavefront reduction, the 16 wavefronts in sequence; reduce_partials in
// fused_common.h strides by 256 and adds four wavefronts pairwise, so the two agree up to the order of additions) -- the
// one-workgroup ggcn_overlap_reduce launch rides along: at a 512-graph shard the two tail launches were 13 us of a 95 us step,
// this one is ~4.
// ggcn_dense_head_signal: the launch counts itself done in memory.  signal[0] collects the workgroups of this launch (every
// workgroup's results are fenced before it arrives; the last arriver clears it for the next launch), signal[1] counts finished
// launches -- a stream gated on it by hipStreamWaitValue32(>= n) may read the logits and xy of the n-th launch without an event
// record on the launching stream (the sharded step: shard.PooledGather, `flag` hand-off).
__device__ __forceinline__ void head_signal(unsigned *__restrict__ signal, int tid)
{
    if (!signal) return;   // kernel-uniform
    __syncthreads();       // every store of this workgroup has been issued
    if (tid == 0) {
        __threadfence_system();
        if (atomicAdd(signal, 1u) == gridDim.x - 1) {
            signal[0] = 0u;
            __threadfence_system();
            atomicAdd_system(signal + 1, 1u);
        }
    }
}

constexpr int kHeadRows = 8, kHeadThreads = 1024, kHeadWaves = kHeadThreads / 64;
static_assert(kHeadWaves == 2 * kHeadRows, "two wavefronts stage a pooled row");
__global__ __launch_bounds__(kHeadThreads) void dense_head_kernel(const float *__restrict__ pooled, int64_t ldp, const float *__restrict__ Wt,
                                                                  int64_t ldw, const float *__restrict__ bias, int B, int H, int C,
                                                                  float *__restrict__ logits, int64_t ldl, const float *__restrict__ part,
                                                                  int n_part, float *__restrict__ xy, int head_blocks, unsigned *__restrict__ signal)
{
    extern __shared__ __attribute__((aligned(16))) float head_lds[];   // [kHeadRows][H] pooled rows, then [kHeadWaves][kHeadRows][64] partial sums
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if ((int)blockIdx.x >= head_blocks) {   // the regulariser's final sum (one workgroup; fixed order: deterministic)
        float sdot = 0.0f;
        for (int idx = tid; idx < n_part; idx += kHeadThreads) sdot += part[idx];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sdot += __shfl_xor(sdot, d);
        if (lane == 0) head_lds[wave] = sdot;
        __syncthreads();
        if (tid == 0) {
            float t = 0.0f;
#pragma unroll
            for (int w = 0; w < kHeadWaves; ++w) t += head_lds[w];
            *xy = t / (float)B;
        }
        head_signal(signal, tid);
        return;
    }
    const int b0 = blockIdx.x * kHeadRows;
    float *rows = head_lds, *red = head_lds + kHeadRows * H;
    {   // the workgroup's pooled rows, read once and coalesced: wavefront (r, half) brings half of row r (no division by H)
        const int r = wave >> 1, hb = (H + 1) >> 1, kb = (wave & 1) * hb, ke = kb + hb < H ? kb + hb : H;
        const bool live = b0 + r < B;
        const float *src = pooled + (int64_t)(live ? b0 + r : 0) * ldp;
        // 16 bytes at a time for H % 8 == 0 alone: both halves are then whole float4s.  (hb % 4 == 0 also holds for H = 8m - 1,
        // where the second half's last float4 would take the pad column and store it on the next row's first element.)
        if ((H & 7) == 0 && (ldp & 3) == 0 && (reinterpret_cast<uintptr_t>(pooled) & 15u) == 0) {
            for (int k = kb + 4 * lane; k < ke; k += 256) {
                const float4 v = *reinterpret_cast<const float4 *>(src + k);
                *reinterpret_cast<float4 *>(rows + r * H + k) = live ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        } else {
            for (int k = kb + lane; k < ke; k += 64) rows[r * H + k] = live ? src[k] : 0.0f;
        }
    }
    __syncthreads();
    // lane = class, wavefront w = k-slice w of 16: every Wt row of the slice is one coalesced load, all of them independent
    const int kq = (H + kHeadWaves - 1) / kHeadWaves, k0 = wave * kq, k1 = k0 + kq < H ? k0 + kq : H;
    const int c = lane < C ? lane : 0;
    float acc[kHeadRows] = {};
    if ((H & 3) == 0 && (kq & 3) == 0) {   // four k per step: one 16-byte LDS broadcast read per row instead of four 4-byte ones
#pragma unroll 4
        for (int k = k0; k < k1; k += 4) {
            float w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = Wt[(int64_t)(k + q) * ldw + c];
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) {
                const float4 xv = *reinterpret_cast<const float4 *>(rows + r * H + k);
                acc[r] = fmaf(xv.x, w[0], acc[r]); acc[r] = fmaf(xv.y, w[1], acc[r]);     // (k ascending: the order of the scalar loop)
                acc[r] = fmaf(xv.z, w[2], acc[r]); acc[r] = fmaf(xv.w, w[3], acc[r]);
            }
        }
    } else {
#pragma unroll 8
        for (int k = k0; k < k1; ++k) {
            const float w = Wt[(int64_t)k * ldw + c];
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) acc[r] = fmaf(rows[r * H + k], w, acc[r]);   // (an LDS broadcast read)
        }
    }
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) red[(wave * kHeadRows + r) * 64 + lane] = acc[r];
    __syncthreads();
    if (wave < kHeadRows && lane < C && b0 + wave < B) {   // wavefront r finishes row r: the 16 slices in ascending order
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < kHeadWaves; ++w) t += red[(w * kHeadRows + wave) * 64 + lane];
        logits[(int64_t)(b0 + wave) * ldl + lane] = t + (bias ? bias[lane] : 0.0f);
    }
    head_signal(signal, tid);
}

}  // namespace

// ggcn_gate_mlp (save = false) and ggcn_gate_mlp_save: the same checks under the entry's own name, the same launch geometry
static int gate_mlp_launch(const char *who, bool save, const float *aspect, int64_t lda, int B, int H, const float *w1t_a,
                           const float *b1_a, const float *w2t_a, const float *b2_a, float *gate_a, const float *w1t_b,
                           const float *b1_b, const float *w2t_b, const float *b2_b, float *gate_b, float *hid_a, float *hid_b,
                           hipStream_t st)
{
    if (!aspect || !w1t_a || !w2t_a || !gate_a || (save && !hid_a)) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if ((gate_b != nullptr) != (w1t_b != nullptr && w2t_b != nullptr))
        return fail(GGCN_EINVAL, "%s: the second gate needs both of its weights and its output (or none)", who);
    if (save && (gate_b != nullptr) != (hid_b != nullptr))
        return fail(GGCN_EINVAL, "%s: hid_b goes with the second gate", who);
    if (B <= 0 || H <= 0 || lda < H) return fail(GGCN_EINVAL, "%s: B=%d H=%d lda=%lld", who, B, H, (long long)lda);
    const size_t lds = (size_t)2 * kGateRows * H * sizeof(float);
    if (lds > 64 * 1024) return fail(GGCN_EUNSUPPORTED, "%s: H=%d needs more than 64 KiB of LDS", who, H);
    GateParams ga{w1t_a, b1_a, w2t_a, b2_a, gate_a, hid_a}, gb{w1t_b, b1_b, w2t_b, b2_b, gate_b, hid_b};
    hipLaunchKernelGGL(save ? gate_mlp_kernel<true> : gate_mlp_kernel<false>,
                       dim3((unsigned)((B + kGateRows - 1) / kGateRows), gate_b ? 2u : 1u), dim3(256), lds, st, aspect, lda, B, H, ga, gb);
    return check_launch(who);
}

// ggcn_dense_head and, with its signal words, ggcn_dense_head_signal (capi.hip)
int dense_head(const float *pooled, int64_t ldp, const float *Wt, int64_t ldw, const float *bias, int B, int H, int C,
               float *logits, int64_t ldl, const float *partials, int F_block, float *xy, hipStream_t st, unsigned *signal)
{
    if (!pooled || !Wt || !logits) return fail(GGCN_EINVAL, "ggcn_dense_head: null pointer");
    if ((partials != nullptr) != (xy != nullptr)) return fail(GGCN_EINVAL, "ggcn_dense_head: overlap_partials and xy go together");
    if (B <= 0 || H <= 0 || C <= 0 || (partials && F_block <= 0)) return fail(GGCN_EINVAL, "ggcn_dense_head: B=%d H=%d C=%d F_block=%d", B, H, C, F_block);
    if (C > 64) return fail(GGCN_EUNSUPPORTED, "ggcn_dense_head: C=%d classes (one lane per class: at most 64)", C);
    if (ldp < H || ldw < C || ldl < C) return fail(GGCN_EINVAL, "ggcn_dense_head: leading dimension too small");
    const int head_blocks = (B + kHeadRows - 1) / kHeadRows;
    const size_t lds = ((size_t)kHeadRows * H + (size_t)kHeadWaves * kHeadRows * 64) * sizeof(float);
    if (lds > 64 * 1024) return fail(GGCN_EUNSUPPORTED, "ggcn_dense_head: H=%d needs more than 64 KiB of LDS", H);
    hipLaunchKernelGGL(dense_head_kernel, dim3((unsigned)(head_blocks + (partials ? 1 : 0))), dim3(kHeadThreads), lds, st, pooled, ldp, Wt, ldw, bias,
                       B, H, C, logits, ldl, partials, partials ? B * ((F_block + 63) / 64) : 0, xy, head_blocks, signal);
    return check_launch("ggcn_dense_head");
}

}  // namespace ggcn

using namespace ggcn;

extern "C" {

int ggcn_transpose(const float *W, int rows, int cols, int64_t ldw, float *Wt, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    if (!W || !Wt) return fail(GGCN_EINVAL, "ggcn_transpose: null pointer");
    if (rows <= 0 || cols <= 0 || ldw < cols) return fail(GGCN_EINVAL, "ggcn_transpose: rows=%d cols=%d ldw=%lld", rows, cols, (long long)ldw);
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, st,
                       W, rows, cols, ldw, Wt);
    return check_launch("ggcn_transpose");
}

int ggcn_gate_mlp(const float *aspect, int64_t lda, int B, int H, const float *w1t_a, const float *b1_a, const float *w2t_a,
                  const float *b2_a, float *gate_a, const float *w1t_b, const float *b1_b, const float *w2t_b,
                  const float *b2_b, float *gate_b, ggcn_stream_t stream)
{
    return gate_mlp_launch("ggcn_gate_mlp", false, aspect, lda, B, H, w1t_a, b1_a, w2t_a, b2_a, gate_a, w1t_b, b1_b, w2t_b, b2_b, gate_b,
                           nullptr, nullptr, as_stream(stream));
}

int ggcn_gate_mlp_save(const float *aspect, int64_t lda, int B, int H, const float *w1t_a, const float *b1_a, const float *w2t_a,
                       const float *b2_a, float *gate_a, const float *w1t_b, const float *b1_b, const float *w2t_b,
                       const float *b2_b, float *gate_b, float *hid_a, float *hid_b, ggcn_stream_t stream)
{
    return gate_mlp_launch("ggcn_gate_mlp_save", true, aspect, lda, B, H, w1t_a, b1_a, w2t_a, b2_a, gate_a, w1t_b, b1_b, w2t_b, b2_b,
                           gate_b, hid_a, hid_b, as_stream(stream));
}

int ggcn_gate_mlp_backward(const float *aspect, int64_t lda, int B, int H, const float *w1_a, const float *w2_a, const float *hid_a,
                           const float *gate_a, const float *d_gate_a, const float *w1_b, const float *w2_b, const float *hid_b,
                           const float *gate_b, const float *d_gate_b, float *d_aspect, int64_t ldda, float *Z, int64_t ldz,
                           ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    if (!aspect) return fail(GGCN_EINVAL, "ggcn_gate_mlp_backward: null pointer");
    if (!d_gate_a && !d_gate_b) return fail(GGCN_EINVAL, "ggcn_gate_mlp_backward: no incoming gradient (both d_gate are NULL)");
    if (!d_aspect && !Z) return fail(GGCN_EINVAL, "ggcn_gate_mlp_backward: nothing to compute (d_aspect and Z are NULL)");
    if ((d_gate_a && (!w2_a || !hid_a || !gate_a || (d_aspect && !w1_a))) || (d_gate_b && (!w2_b || !hid_b || !gate_b || (d_aspect && !w1_b))))
        return fail(GGCN_EINVAL, "ggcn_gate_mlp_backward: a gate with a gradient needs its weights, hid and gate");
    if (B <= 0 || H <= 0) return fail(GGCN_EINVAL, "ggcn_gate_mlp_backward: B=%d H=%d", B, H);
    const int64_t Hp = ((int64_t)H + 3) & ~(int64_t)3;
    if (lda < H || (d_aspect && ldda < H) || (Z && ldz < 5 * Hp))
        return fail(GGCN_EINVAL, "ggcn_gate_mlp_backward: leading dimension too small");
    const size_t lds = (size_t)2 * kGateRows * H * sizeof(float);
    if (lds > 64 * 1024) return fail(GGCN_EUNSUPPORTED, "ggcn_gate_mlp_backward: H=%d needs more than 64 KiB of LDS", H);
    GateGrad ga{w1_a, w2_a, hid_a, gate_a, d_gate_a}, gb{w1_b, w2_b, hid_b, gate_b, d_gate_b};
    const bool vec = (H & 3) == 0;
    const int nc = (H + 255) / 256;   // 1..4 under the LDS bound
    auto kernel = nc == 1 ? (vec ? gate_mlp_backward_kernel<true, 1> : gate_mlp_backward_kernel<false, 1>)
                : nc == 2 ? (vec ? gate_mlp_backward_kernel<true, 2> : gate_mlp_backward_kernel<false, 2>)
                : nc == 3 ? (vec ? gate_mlp_backward_kernel<true, 3> : gate_mlp_backward_kernel<false, 3>)
                          : (vec ? gate_mlp_backward_kernel<true, 4> : gate_mlp_backward_kernel<false, 4>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + kGateRows - 1) / kGateRows)), dim3(256), lds, st, aspect, lda, B, H, ga, gb, d_aspect,
                       ldda, Z, ldz);
    return check_launch("ggcn_gate_mlp_backward");
}

int ggcn_scores_head(const float *X, int64_t ldx, const float *aspect, int64_t lda, const float *logits, int64_t ldl,
                     const float *fcw, int64_t ldw, const float *fcb, const float *dist, int64_t ldd, int B, int T, int H,
                     int C, float *scores, int64_t lds_, float *kl_part, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    if (!X || !aspect || !logits || !fcw || !scores) return fail(GGCN_EINVAL, "ggcn_scores_head: null pointer");
    if ((kl_part != nullptr) != (dist != nullptr)) return fail(GGCN_EINVAL, "ggcn_scores_head: dist and kl_part go together");
    if (B <= 0 || T <= 0 || H <= 0 || C <= 0) return fail(GGCN_EINVAL, "ggcn_scores_head: B=%d T=%d H=%d C=%d", B, T, H, C);
    if (ldx < H || lda < H || ldl < C || ldw < 2 * H || lds_ < T || (dist && ldd < T))
        return fail(GGCN_EINVAL, "ggcn_scores_head: leading dimension too small");
    const size_t lds = (size_t)(H + C + T + 8) * sizeof(float);
    if (lds > 64 * 1024) return fail(GGCN_EUNSUPPORTED, "ggcn_scores_head: H + C + T = %d needs more than 64 KiB of LDS", H + C + T);
    hipLaunchKernelGGL(scores_head_kernel, dim3((unsigned)B), dim3(256), lds, st, X, ldx, aspect, lda, logits, ldl, fcw, ldw,
                       fcb, dist, ldd, T, H, C, scores, lds_, kl_part);
    return check_launch("ggcn_scores_head");
}

int ggcn_scores_head_backward(const float *X, int64_t ldx, const float *aspect, int64_t lda, const float *logits, int64_t ldl,
                              const float *fcw, int64_t ldw, const float *fcb, const float *dist, int64_t ldd, const float *scores,
                              int64_t lds_, const float *kl_part, const float *g_scores, int64_t ldgs, const float *g_kl, int B, int T,
                              int H, int C, float *dX, int64_t lddx, float *d_aspect, int64_t ldda, float *d_logits, int64_t lddl,
                              float *G, int64_t ldg, float *dc0, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    if (!X || !aspect || !logits || !fcw) return fail(GGCN_EINVAL, "ggcn_scores_head_backward: null pointer");
    if (g_kl && (!dist || !scores || !kl_part))
        return fail(GGCN_EINVAL, "ggcn_scores_head_backward: a gradient of kl needs dist, the saved scores and the saved kl_part");
    if ((G != nullptr) != (dc0 != nullptr)) return fail(GGCN_EINVAL, "ggcn_scores_head_backward: G and dc0 go together");
    if (B <= 0 || T <= 0 || H <= 0 || C <= 0) return fail(GGCN_EINVAL, "ggcn_scores_head_backward: B=%d T=%d H=%d C=%d", B, T, H, C);
    if (ldx < H || lda < H || ldl < C || ldw < 2 * H || (g_kl && (ldd < T || lds_ < T)) || (g_scores && ldgs < T) || (dX && lddx < H) ||
        (d_aspect && ldda < H) || (d_logits && lddl < C) || (G && ldg < 2 * H))
        return fail(GGCN_EINVAL, "ggcn_scores_head_backward: leading dimension too small");
    const size_t lds = ((size_t)6 * ((H + 3) & ~3) + C + T + 8) * sizeof(float);
    if (lds > 64 * 1024)
        return fail(GGCN_EUNSUPPORTED, "ggcn_scores_head_backward: 6 H + C + T = %lld floats need more than 64 KiB of LDS",
                    6LL * H + C + T);
    const auto aligned16 = [](const void *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (ld & 3) == 0; };
    const bool vec = (H & 3) == 0 && aligned16(X, ldx) && (!dX || aligned16(dX, lddx));
    hipLaunchKernelGGL(vec ? scores_head_backward_kernel<true> : scores_head_backward_kernel<false>, dim3((unsigned)B), dim3(256), lds, st,
                       X, ldx, aspect, lda, logits, ldl, fcw, ldw, fcb, dist, ldd, scores, lds_, kl_part, g_scores, ldgs, g_kl, B, T, H, C,
                       dX, lddx, d_aspect, ldda, d_logits, lddl, G, ldg, dc0);
    return check_launch("ggcn_scores_head_backward");
}

size_t ggcn_scores_head_dweight_workspace_bytes(int B, int H, int C)
{
    if (B <= 0 || H <= 0 || C <= 0) return sizeof(float);
    return (size_t)((B + kDwRows - 1) / kDwRows) * (size_t)C * (size_t)(2 * H + 1) * sizeof(float);
}

int ggcn_scores_head_dweight(const float *logits, int64_t ldl, const float *G, int64_t ldg, const float *dc0, int B, int H, int C,
                             float *dW, int64_t lddw, float *d_bias, void *workspace, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    if (!logits || !G || !dc0 || !dW || !workspace) return fail(GGCN_EINVAL, "ggcn_scores_head_dweight: null pointer");
    if (B <= 0 || H <= 0 || C <= 0) return fail(GGCN_EINVAL, "ggcn_scores_head_dweight: B=%d H=%d C=%d", B, H, C);
    if (ldl < C || ldg < 2 * H || lddw < 2 * H) return fail(GGCN_EINVAL, "ggcn_scores_head_dweight: leading dimension too small");
    const int W2 = 2 * H, slices = (B + kDwRows - 1) / kDwRows;
    if (slices > 65535) return fail(GGCN_EUNSUPPORTED, "ggcn_scores_head_dweight: B=%d (at most %d sentences)", B, 65535 * kDwRows);
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(head_dweight_partial_kernel, dim3((unsigned)((W2 + 1 + 255) / 256), (unsigned)((C + kDwClasses - 1) / kDwClasses), (unsigned)slices),
                       dim3(256), 0, st, logits, ldl, G, ldg, dc0, B, W2, C, part);
    const int64_t n = (int64_t)C * (W2 + 1);
    hipLaunchKernelGGL(head_dweight_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, slices, W2, C, dW, lddw, d_bias);
    return check_launch("ggcn_scores_head_dweight");
}

}  // extern "C"
