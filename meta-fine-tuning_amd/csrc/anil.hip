// ANIL head: K gradient steps on a linear classifier over the support rows of an episode, and the exact
// second-order backward through them.  Every episode of a step per launch.  Forward: anil_chain_kernel<false> (one workgroup per
// episode walks the K dependent steps and writes the tape W_t, b_t, P_t), anil_scores_kernel.  Backward: anil_scores_grad_kernel
// (dZ_Q and the episode's gW, gb at t = K), anil_chain_kernel<true> (the reverse recursion: the same walk with the softmax Jacobian
// in the place of the softmax; tape gW_t, gb_t, R_t), anil_support_grad_kernel (dZ_S from the four tapes, many workgroups, and the
// sum of the episodes' gW_0, gb_0 in episode order).
//
// fp32 storage, every sum in double, fixed summation order, no atomics, every output element written once.  The walk keeps its
// [n_way][512] matrix (W_t forward, gW_t backward) twice: as doubles in registers, 16 classes of one column per thread, which
// take the K updates, and rounded to fp32 in LDS and on the tape, which the row products read.  Z_S is read from L2 in every step.
#include <math.h>
#include "ridge_common.h"

namespace {

constexpr int ANIL_MAX_STEPS = 16;
constexpr int ANIL_ROWS = 8;                        // rows per workgroup of the two row-gradient launches
constexpr int ANIL_COLB = RIDGE_D / RIDGE_THREADS;  // columns per thread there
static_assert(RIDGE_WG == 2 * RIDGE_D && RIDGE_MAX_WAY == 32, "the walk: one column and 16 of the 32 classes per thread");
static_assert(ANIL_COLB == 2, "two columns per thread");

// LDS of the walk: the matrix [n_way][512] fp32, the panel [S][16 or 32] fp32 (P_t - Y forward, R_t backward; the columns past n_way
// stay zero, so that the update adds 16 classes per thread without a test), the bias [32] double
__host__ __device__ inline int anil_panel_ld(int n_way) { return n_way <= 16 ? 16 : 32; }
inline size_t anil_chain_lds(int S, int n_way) { return 4 * ((size_t)n_way * RIDGE_D + (size_t)S * anil_panel_ld(n_way)) + 8 * RIDGE_MAX_WAY; }
constexpr int ANIL_MAX_LDS = 4 * (RIDGE_MAX_WAY * RIDGE_D + RIDGE_MAX_S * RIDGE_MAX_WAY) + 8 * RIDGE_MAX_WAY;
static_assert(ANIL_MAX_LDS <= 160 * 1024, "one CU's LDS");

// ---------------------------------------------------------------------------------------------------------------- the walk
// BWD = false: slot 0 of (Mt, vt) = (M0, v0); for t = 0 .. K-1: P_t = softmax(Z_S M_t^T + v_t) (stored if P is given), panel =
//              P_t - Y, slot t + 1 = slot t - aS panel^T Z_S, - aS sum_rows panel.
// BWD = true:  slot K of (Mt, vt) is there; for t = K-1 .. 0: U = Z_S M_{t+1}^T + v_{t+1}, panel = R_t = P_t * (U - rowsum(P_t * U))
//              (stored in R), slot t = slot t + 1 - aS panel^T Z_S, - aS sum_rows panel.
template <bool BWD>
__global__ __launch_bounds__(RIDGE_WG) void anil_chain_kernel(const float* __restrict__ feats, RidgeShape s, int K, double aS,
                                                              const float* __restrict__ M0, const float* __restrict__ v0,
                                                              float* __restrict__ Mt, float* __restrict__ vt, float* __restrict__ P,
                                                              float* __restrict__ R) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = s.n_way, S = C * s.ns, CP = anil_panel_ld(C);
    float* sm = (float*)smem;
    const f32x4* sm4 = (const f32x4*)smem;
    float* sr = sm + C * RIDGE_D;
    double* sv = (double*)(sr + S * CP);
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = tid & (RIDGE_D - 1), c0 = (tid >> 9) * 16;
    const float* ep = feats + (long long)e * C * (s.ns + s.nq) * s.ld;
    float* Me = Mt + (long long)e * (K + 1) * C * RIDGE_D;
    float* ve = vt + (long long)e * (K + 1) * C;
    float* Pe = P == nullptr ? nullptr : P + (long long)e * K * S * C;
    float* Re = R == nullptr ? nullptr : R + (long long)e * K * S * C;

    // (a thread's slots past n_way hold a copy of the last class: their panel columns are zero and they are never stored)
    double m[16], mv = 0.0;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) {
        const int at = min(c0 + cc, C - 1) * RIDGE_D + d;
        const float w = BWD ? Me[(long long)K * C * RIDGE_D + at] : M0[at];
        m[cc] = (double)w;
        if (c0 + cc < C) {
            sm[at] = w;
            if (!BWD) Me[at] = w;
        }
    }
    for (int i = tid; i < S * CP; i += RIDGE_WG) sr[i] = 0.f;
    if (tid < C) {
        const float b = BWD ? ve[K * C + tid] : v0[tid];
        mv = (double)b;
        sv[tid] = (double)b;
        if (!BWD) ve[tid] = b;
    }
    __syncthreads();

    for (int step = 0; step < K; ++step) {
        const int t = BWD ? K - 1 - step : step;                   // the softmax of this step is P_t
        const int to = BWD ? t : t + 1;                            // the slot this step writes
        // rows wave, wave + 16, ...: lane c ends up with the row's product with class c
        for (int i = wave; i < S; i += RIDGE_WG / 64) {            // uniform over the wave
            const float* x = sup_row(ep, s, i);
            const f32x4 x0 = *(const f32x4*)(x + 4 * lane), x1 = *(const f32x4*)(x + 256 + 4 * lane);
            double mine = 0.0;
            for (int k = 0; k < C; ++k) {
                const double p = group_sum<64>(dot4(x0, sm4[k * 128 + lane]) + dot4(x1, sm4[k * 128 + 64 + lane]));
                if (lane == k) mine = p + sv[k];
            }
            const long long at = ((long long)t * S + i) * C + lane;
            if (!BWD) {
                double mx = lane < C ? mine : -INFINITY;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
                const double ex = lane < C ? exp(mine - mx) : 0.0;
                const float p = (float)(ex / group_sum<64>(ex));
                if (lane < C) {
                    if (Pe != nullptr) Pe[at] = p;
                    sr[i * CP + lane] = (float)((double)p - (lane == i / s.ns ? 1.0 : 0.0));
                }
            } else {
                const double p = lane < C ? (double)Pe[at] : 0.0;
                const double u = lane < C ? mine : 0.0;
                const float r = (float)(p * (u - group_sum<64>(p * u)));
                if (lane < C) {
                    Re[at] = r;
                    sr[i * CP + lane] = r;
                }
            }
        }
        __syncthreads();
        // column d, classes c0 .. c0 + 15: the update in the double copy, then its rounding into LDS and onto the tape
        if (c0 < C) {
            for (int i = 0; i < S; ++i) {
                const double z = aS * (double)sup_row(ep, s, i)[d];
                const f32x4* r = (const f32x4*)(sr + i * CP + c0);
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const f32x4 r4 = r[cc];
                    m[4 * cc] -= z * (double)r4.x;
                    m[4 * cc + 1] -= z * (double)r4.y;
                    m[4 * cc + 2] -= z * (double)r4.z;
                    m[4 * cc + 3] -= z * (double)r4.w;
                }
            }
#pragma unroll
            for (int cc = 0; cc < 16; ++cc)
                if (c0 + cc < C) {
                    const int at = (c0 + cc) * RIDGE_D + d;
                    const float w = (float)m[cc];
                    sm[at] = w;
                    Me[(long long)to * C * RIDGE_D + at] = w;
                }
        }
        if (tid < C) {
            double acc = 0.0;
            for (int i = 0; i < S; ++i) acc += (double)sr[i * CP + tid];
            mv -= aS * acc;
            const float b = (float)mv;
            sv[tid] = (double)b;
            ve[to * C + tid] = b;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- scores
// 16 query rows per workgroup, one wave per row; W_K in LDS in chunks of 16 classes; lane c keeps the row's score of class c
__global__ __launch_bounds__(RIDGE_THREADS) void anil_scores_kernel(const float* __restrict__ feats, RidgeShape s, int K,
                                                                    const float* __restrict__ Wt, const float* __restrict__ bt,
                                                                    float* __restrict__ scores) {
    __shared__ f32x4 sw[16 * RIDGE_D / 4];
    const int e = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qrows = s.n_way * s.nq;
    const float* ep = feats + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
    const f32x4* We = (const f32x4*)(Wt + ((long long)e * (K + 1) + K) * s.n_way * RIDGE_D);
    const float* be = bt + ((long long)e * (K + 1) + K) * s.n_way;
    float* out = scores + (long long)e * qrows * s.n_way;
    float mine[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < s.n_way; c0 += 16) {
        const int cb = min(16, s.n_way - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < cb * (RIDGE_D / 4); i += RIDGE_THREADS) sw[i] = We[c0 * (RIDGE_D / 4) + i];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int r = blockIdx.x * 16 + wave + 4 * m;
            if (r >= qrows) continue;                            // uniform over the wave
            const float* x = ep + qry_row(s, r) * s.ld;
            const f32x4 x0 = *(const f32x4*)(x + 4 * lane), x1 = *(const f32x4*)(x + 256 + 4 * lane);
            for (int k = 0; k < cb; ++k) {
                const double p = group_sum<64>(dot4(x0, sw[k * 128 + lane]) + dot4(x1, sw[k * 128 + 64 + lane]));
                if (lane == c0 + k) mine[m] = (float)((double)be[c0 + k] + p);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = blockIdx.x * 16 + wave + 4 * m;
        if (r < qrows && lane < s.n_way) out[(long long)r * s.n_way + lane] = mine[m];
    }
}

// ---------------------------------------------------------------------------------------------------------------- scores backward
// blockIdx.x < 4: slot K of gWt = G^T Z_Q for 256 columns and 16 classes, the query rows in order (block 0 also slot K of gbt);
// the other workgroups: dZ_Q = G W_K for ANIL_ROWS query rows each, two columns per thread
__global__ __launch_bounds__(RIDGE_THREADS) void anil_scores_grad_kernel(const float* __restrict__ feats, RidgeShape s, int K,
                                                                         const float* __restrict__ Wt, const float* __restrict__ G,
                                                                         float* __restrict__ dfeats, int ldd, float* __restrict__ gWt,
                                                                         float* __restrict__ gbt) {
    __shared__ float sg[ANIL_ROWS * RIDGE_MAX_WAY];
    const int e = blockIdx.y, tid = threadIdx.x, C = s.n_way, Q = C * s.nq;
    const long long row0 = (long long)e * C * (s.ns + s.nq);
    const float* ep = feats + row0 * s.ld;
    const float* Ge = G + (long long)e * Q * C;
    if (blockIdx.x < 4) {
        const int d = (blockIdx.x & 1) * RIDGE_THREADS + tid, c0 = (blockIdx.x >> 1) * 16;
        if (c0 >= C) return;
        double acc[16];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) acc[cc] = 0.0;
        for (int r = 0; r < Q; ++r) {
            const double z = ep[qry_row(s, r) * s.ld + d];
            const float* g = Ge + (long long)r * C + c0;
#pragma unroll
            for (int cc = 0; cc < 16; ++cc)
                if (c0 + cc < C) acc[cc] += z * (double)g[cc];
        }
        float* out = gWt + ((long long)e * (K + 1) + K) * C * RIDGE_D;
#pragma unroll
        for (int cc = 0; cc < 16; ++cc)
            if (c0 + cc < C) out[(c0 + cc) * RIDGE_D + d] = (float)acc[cc];
        if (blockIdx.x == 0 && tid < C) {
            double sum = 0.0;
            for (int r = 0; r < Q; ++r) sum += (double)Ge[(long long)r * C + tid];
            gbt[((long long)e * (K + 1) + K) * C + tid] = (float)sum;
        }
        return;
    }
    const int r0 = (blockIdx.x - 4) * ANIL_ROWS;
    for (int i = tid; i < ANIL_ROWS * C; i += RIDGE_THREADS) {
        const int r = r0 + i / C;
        sg[i] = r < Q ? Ge[(long long)r * C + (i - (i / C) * C)] : 0.f;
    }
    __syncthreads();
    const float* We = Wt + ((long long)e * (K + 1) + K) * C * RIDGE_D;
    double acc[ANIL_ROWS][ANIL_COLB];
#pragma unroll
    for (int q = 0; q < ANIL_ROWS; ++q) acc[q][0] = acc[q][1] = 0.0;
    for (int c = 0; c < C; ++c) {
        const double w0 = We[c * RIDGE_D + tid], w1 = We[c * RIDGE_D + RIDGE_THREADS + tid];
#pragma unroll
        for (int q = 0; q < ANIL_ROWS; ++q) {
            const double g = sg[q * C + c];
            acc[q][0] += g * w0;
            acc[q][1] += g * w1;
        }
    }
#pragma unroll
    for (int q = 0; q < ANIL_ROWS; ++q) {
        const int r = r0 + q;
        if (r < Q) {
            float* o = dfeats + (row0 + qry_row(s, r)) * ldd;
            o[tid] = (float)acc[q][0];
            o[RIDGE_THREADS + tid] = (float)acc[q][1];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- support gradient
// The first episodes * row_blocks workgroups, row_blocks per episode: dZ_S of ANIL_ROWS support rows = -aS sum_t ((P_t - Y) gW_{t+1}
// + R_t W_t), t descending, classes in order, two columns per thread; the coefficients of all steps are staged in LDS first.  The
// workgroups behind them: dW0, db0 = slot 0 of gWt, gbt added over the episodes in order.
__global__ __launch_bounds__(RIDGE_THREADS) void anil_support_grad_kernel(RidgeShape s, int K, int episodes, double aS, int row_blocks,
                                                                          const float* __restrict__ Wt, const float* __restrict__ P,
                                                                          const float* __restrict__ gWt, const float* __restrict__ gbt,
                                                                          const float* __restrict__ R, float* __restrict__ dfeats, int ldd,
                                                                          float* __restrict__ dW0, float* __restrict__ db0) {
    __shared__ float sp[ANIL_MAX_STEPS * ANIL_ROWS * RIDGE_MAX_WAY];
    __shared__ float sr[ANIL_MAX_STEPS * ANIL_ROWS * RIDGE_MAX_WAY];
    const int bx = blockIdx.x, e = bx / row_blocks, tid = threadIdx.x, C = s.n_way, S = C * s.ns;
    const long long slot = (long long)C * RIDGE_D;
    if (e >= episodes) {
        const long long j = (long long)(bx - episodes * row_blocks) * RIDGE_THREADS + tid;
        if (j < slot) {
            double acc = 0.0;
            for (int ee = 0; ee < episodes; ++ee) acc += (double)gWt[(long long)ee * (K + 1) * slot + j];
            dW0[j] = (float)acc;
        } else if (j < slot + C) {
            const int c = (int)(j - slot);
            double acc = 0.0;
            for (int ee = 0; ee < episodes; ++ee) acc += (double)gbt[(long long)ee * (K + 1) * C + c];
            db0[c] = (float)acc;
        }
        return;
    }
    const int i0 = (bx - e * row_blocks) * ANIL_ROWS;
    const float* Pe = P + (long long)e * K * S * C;
    const float* Re = R + (long long)e * K * S * C;
    for (int idx = tid; idx < K * ANIL_ROWS * C; idx += RIDGE_THREADS) {
        const int t = idx / (ANIL_ROWS * C), rem = idx - t * (ANIL_ROWS * C), q = rem / C, c = rem - q * C, i = i0 + q;
        float p = 0.f, r = 0.f;
        if (i < S) {
            const long long at = ((long long)t * S + i) * C + c;
            p = (float)((double)Pe[at] - (c == i / s.ns ? 1.0 : 0.0));
            r = Re[at];
        }
        sp[idx] = p;
        sr[idx] = r;
    }
    __syncthreads();
    const float* We = Wt + (long long)e * (K + 1) * slot;
    const float* gWe = gWt + (long long)e * (K + 1) * slot;
    double acc[ANIL_ROWS][ANIL_COLB];
#pragma unroll
    for (int q = 0; q < ANIL_ROWS; ++q) acc[q][0] = acc[q][1] = 0.0;
    for (int t = K - 1; t >= 0; --t)
        for (int c = 0; c < C; ++c) {
            const float* gw = gWe + (long long)(t + 1) * slot + c * RIDGE_D;
            const float* w = We + (long long)t * slot + c * RIDGE_D;
            const double g0 = gw[tid], g1 = gw[RIDGE_THREADS + tid], w0 = w[tid], w1 = w[RIDGE_THREADS + tid];
#pragma unroll
            for (int q = 0; q < ANIL_ROWS; ++q) {
                const double p = sp[(t * ANIL_ROWS + q) * C + c], r = sr[(t * ANIL_ROWS + q) * C + c];
                acc[q][0] += p * g0 + r * w0;
                acc[q][1] += p * g1 + r * w1;
            }
        }
    const long long row0 = (long long)e * C * (s.ns + s.nq);
#pragma unroll
    for (int q = 0; q < ANIL_ROWS; ++q) {
        const int i = i0 + q;
        if (i < S) {
            const int cl = i / s.ns;
            float* o = dfeats + (row0 + cl * (s.ns + s.nq) + (i - cl * s.ns)) * ldd;
            o[tid] = (float)(-aS * acc[q][0]);
            o[RIDGE_THREADS + tid] = (float)(-aS * acc[q][1]);
        }
    }
}

inline bool anil_ok(const void* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, int K) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D)) return false;
    if (K < 1 || K > ANIL_MAX_STEPS || episodes > 65535) return false;
    return (long long)episodes * n_way * ((long long)n_support + n_query) < (1ll << 31) / RIDGE_D;
}

inline bool anil_lr_ok(float a) { return a > 0.f && a < INFINITY; }

inline bool anil_aligned(const void* p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }

template <typename Kern>
int anil_lds_attr(Kern kern, MftPerDeviceOnce& once) {
    if (once.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, ANIL_MAX_LDS);
        if (e != hipSuccess) return (int)e;
        once.mark();
    }
    return 0;
}

}  // namespace

extern "C" int mft_anil_adapt(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, const float* W0,
                              const float* b0, int inner_steps, float inner_lr, float* Wt, float* bt, float* P, void* stream) {
    if (!anil_ok(feats, ld, episodes, n_way, n_support, n_query, D, inner_steps) || !anil_lr_ok(inner_lr) || !anil_aligned(W0) ||
        b0 == nullptr || !anil_aligned(Wt) || bt == nullptr)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = anil_lds_attr(anil_chain_kernel<false>, once);
    if (rc != 0) return rc;
    const RidgeShape s{n_way, n_support, n_query, ld};
    const int S = n_way * n_support;
    hipLaunchKernelGGL(anil_chain_kernel<false>, dim3(episodes), dim3(RIDGE_WG), anil_chain_lds(S, n_way), (hipStream_t)stream, feats, s,
                       inner_steps, (double)inner_lr / S, W0, b0, Wt, bt, P, (float*)nullptr);
    return mft_launch_status();
}

extern "C" int mft_anil_scores(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, int inner_steps,
                               const float* Wt, const float* bt, float* scores, void* stream) {
    if (!anil_ok(feats, ld, episodes, n_way, n_support, n_query, D, inner_steps) || !anil_aligned(Wt) || bt == nullptr ||
        scores == nullptr)
        return MFT_EINVAL;
    const RidgeShape s{n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(anil_scores_kernel, dim3(cdiv((long long)n_way * n_query, 16), episodes), dim3(RIDGE_THREADS), 0,
                       (hipStream_t)stream, feats, s, inner_steps, Wt, bt, scores);
    return mft_launch_status();
}

extern "C" int mft_anil_scores_backward(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                        int inner_steps, const float* Wt, const float* dscores, float* dfeats, int ldd, float* gWt,
                                        float* gbt, void* stream) {
    if (!anil_ok(feats, ld, episodes, n_way, n_support, n_query, D, inner_steps) || !anil_aligned(Wt) || dscores == nullptr ||
        !anil_aligned(dfeats) || ldd < D || !anil_aligned(gWt) || gbt == nullptr)
        return MFT_EINVAL;
    const RidgeShape s{n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(anil_scores_grad_kernel, dim3(4 + cdiv((long long)n_way * n_query, ANIL_ROWS), episodes), dim3(RIDGE_THREADS), 0,
                       (hipStream_t)stream, feats, s, inner_steps, Wt, dscores, dfeats, ldd, gWt, gbt);
    return mft_launch_status();
}

extern "C" int mft_anil_adapt_backward(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                       int inner_steps, float inner_lr, const float* Wt, const float* P, float* gWt, float* gbt, float* R,
                                       float* dfeats, int ldd, float* dW0, float* db0, void* stream) {
    if (!anil_ok(feats, ld, episodes, n_way, n_support, n_query, D, inner_steps) || !anil_lr_ok(inner_lr) || !anil_aligned(Wt) ||
        P == nullptr || !anil_aligned(gWt) || gbt == nullptr || R == nullptr || !anil_aligned(dfeats) || ldd < D || !anil_aligned(dW0) ||
        db0 == nullptr)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = anil_lds_attr(anil_chain_kernel<true>, once);
    if (rc != 0) return rc;
    const RidgeShape s{n_way, n_support, n_query, ld};
    const int S = n_way * n_support;
    const double aS = (double)inner_lr / S;
    hipLaunchKernelGGL(anil_chain_kernel<true>, dim3(episodes), dim3(RIDGE_WG), anil_chain_lds(S, n_way), (hipStream_t)stream, feats, s,
                       inner_steps, aS, (const float*)nullptr, (const float*)nullptr, gWt, gbt, const_cast<float*>(P), R);
    const int st = mft_launch_status();
    if (st != 0) return st;
    const int row_blocks = cdiv(S, ANIL_ROWS);
    hipLaunchKernelGGL(anil_support_grad_kernel, dim3(episodes * row_blocks + cdiv((long long)n_way * RIDGE_D + n_way, RIDGE_THREADS)),
                       dim3(RIDGE_THREADS), 0, (hipStream_t)stream, s, inner_steps, episodes, aS, row_blocks, Wt, P, gWt, gbt, R, dfeats,
                       ldd, dW0, db0);
    return mft_launch_status();
}
