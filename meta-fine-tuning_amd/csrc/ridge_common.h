// Episode layout, domain and small device helpers shared by the two MetaOptNet heads: csrc/ridge.hip and
// csrc/svm.hip (section 17).
#pragma once
#include "mft_common.h"

namespace {

constexpr int RIDGE_D = 512;
constexpr int RIDGE_MAX_S = 256;
constexpr int RIDGE_MAX_WAY = 32;
constexpr int RIDGE_WG = 1024;              // factor / support-side launches: one workgroup per episode
constexpr int RIDGE_THREADS = 256;          // gram / scores / query-side launches
constexpr int RIDGE_CB = RIDGE_D / 64;      // 64-column blocks of the query-side launch

struct RidgeShape {
    int n_way, ns, nq, ld;
};

__device__ __forceinline__ const float* sup_row(const float* ep, const RidgeShape s, int i) {
    const int c = i / s.ns;
    return ep + (long long)(c * (s.ns + s.nq) + (i - c * s.ns)) * s.ld;
}

__device__ __forceinline__ long long qry_row(const RidgeShape s, int r) {
    const int c = r / s.nq;
    return (long long)(c * (s.ns + s.nq) + s.ns + (r - c * s.nq));
}

// sum over the 2^bits lanes that differ in the low bits: every lane adds the same pairs, so all of them hold the same bits
template <int LANES>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double dot4(const f32x4 a, const f32x4 b) {
    return (double)a.x * (double)b.x + (double)a.y * (double)b.y + (double)a.z * (double)b.z + (double)a.w * (double)b.w;
}

// out[c][d] = sum_s Z_S[s][d] coef[s][c] for the thread's column d and its 16 classes c0 .. c0 + 15 (coef [S][n_way] in LDS)
__device__ __forceinline__ void support_combine(const float* __restrict__ ep, const RidgeShape s, int S, int d, int c0,
                                                const float* __restrict__ coef, double (&out)[16]) {
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) out[cc] = 0.0;
    if (c0 >= s.n_way) return;
    for (int i = 0; i < S; ++i) {
        const double z = sup_row(ep, s, i)[d];
        const float* cf = coef + i * s.n_way + c0;
#pragma unroll
        for (int cc = 0; cc < 16; ++cc)
            if (c0 + cc < s.n_way) out[cc] += z * (double)cf[cc];
    }
}

// dZ_S = alpha (dW - U)^T - B W^T with U[c] = sum_s B[s][c] Z_S[s], by the 1024 threads of a one-workgroup-per-episode launch:
// sa = alpha and sb = B [S][n_way] are in LDS (and the workgroup has synchronised), sm [n_way][D] is LDS scratch for dW - U
__device__ __forceinline__ void support_assemble(const float* __restrict__ ep, const RidgeShape s, int S, int tid,
                                                 const float* __restrict__ sa, const float* __restrict__ sb, float* __restrict__ sm,
                                                 const float* __restrict__ We, const float* __restrict__ dWe,
                                                 float* __restrict__ dep, int ldd) {
    const int d = tid & (RIDGE_D - 1), half = tid >> 9, c0 = half * 16;
    {
        double u[16];
        support_combine(ep, s, S, d, c0, sb, u);
#pragma unroll
        for (int cc = 0; cc < 16; ++cc)
            if (c0 + cc < s.n_way) sm[(c0 + cc) * RIDGE_D + d] = (float)((double)dWe[(c0 + cc) * RIDGE_D + d] - u[cc]);
    }
    __syncthreads();
    // support rows half, half + 2, ... eight at a time: each class's column entries are read once per eight rows
    for (int i0 = half; i0 < S; i0 += 16) {
        double acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.0;
        for (int cc = 0; cc < s.n_way; ++cc) {
            const double m = sm[cc * RIDGE_D + d], w = We[cc * RIDGE_D + d];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int i = i0 + 2 * q;
                if (i < S) acc[q] += (double)sa[i * s.n_way + cc] * m - (double)sb[i * s.n_way + cc] * w;
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = i0 + 2 * q;
            if (i < S) {
                const int cl = i / s.ns;
                dep[(long long)(cl * (s.ns + s.nq) + (i - cl * s.ns)) * ldd + d] = (float)acc[q];
            }
        }
    }
}

inline bool ridge_shape_ok(const void* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D) {
    if (feats == nullptr || episodes < 1 || n_way < 1 || n_way > RIDGE_MAX_WAY || n_support < 1 || n_query < 1) return false;
    if ((long long)n_way * n_support > RIDGE_MAX_S) return false;
    if (D != RIDGE_D || ld < D || (ld & 3) != 0) return false;
    return ((uintptr_t)feats & 15) == 0;
}

}  // namespace
