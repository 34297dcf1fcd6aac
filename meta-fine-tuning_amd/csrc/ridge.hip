// MetaOptNet ridge-regression head forward and backward, every episode of a step in one launch sequence.
//
//   A = Z_S Z_S^T + lambda I    alpha = 2 A^-1 Y    W = Z_S^T alpha    scores = scale * Z_Q W
//
// Layout (as csrc/protonet.hip): feats [episodes, n_way, n_support + n_query, D = 512] with row stride ld; support row s of an
// episode is row (s / n_support) * (n_support + n_query) + s % n_support, Y[s, c] = [s / n_support == c] is computed from the row
// index; scores [episodes * n_way * n_query, n_way], query rows class-major.  Workspaces: A / L [episodes, S, S] (lower triangle
// only), alpha [episodes, S, n_way], W and dW [episodes, n_way, D] (one row per class).
//
// Storage is fp32; every dot product and both triangular solves accumulate in double inside the kernel and round once on the
// store, so each stage is within one fp32 rounding of its exact value on the stored inputs.  No atomics; all sums run in a fixed
// order (butterfly sums add the same pairs in every lane), so two launches on the same input are bit-identical.  No kernel waits
// for another workgroup and every loop is bounded by a shape argument: a non-finite feature gives non-finite output.
#include "ridge_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- Gram
// lower triangle of A = Z_S Z_S^T + lambda I in 32x32 tiles, one tile per workgroup, 2x2 entries per thread
__global__ __launch_bounds__(RIDGE_THREADS) void ridge_gram_kernel(const float* __restrict__ feats, RidgeShape s, int tiles,
                                                                   float lambda_reg, float* __restrict__ A) {
    __shared__ float sa[32][33], sb[32][33];
    const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles;
    if (tj > ti) return;
    const int e = blockIdx.y, S = s.n_way * s.ns;
    const float* ep = feats + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int ia = ti * 32 + lr, ib = tj * 32 + lr;
    const float* pa = ia < S ? sup_row(ep, s, ia) : nullptr;
    const float* pb = ib < S ? sup_row(ep, s, ib) : nullptr;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int k0 = 0; k0 < RIDGE_D; k0 += 32) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 va = pa ? *(const f32x4*)(pa + k0 + lc) : z;
        const f32x4 vb = pb ? *(const f32x4*)(pb + k0 + lc) : z;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sa[lr][lc + q] = va[q];
            sb[lr][lc + q] = vb[q];
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const double a0 = sa[ty][k], a1 = sa[ty + 16][k], b0 = sb[tx][k], b1 = sb[tx + 16][k];
            acc[0][0] += a0 * b0;
            acc[0][1] += a0 * b1;
            acc[1][0] += a1 * b0;
            acc[1][1] += a1 * b1;
        }
    }
    float* Ae = A + (long long)e * S * S;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = ti * 32 + ty + 16 * u, j = tj * 32 + tx + 16 * v;
            if (i < S && j <= i) Ae[(long long)i * S + j] = (float)(acc[u][v] + (i == j ? (double)lambda_reg : 0.0));
        }
}

// ---------------------------------------------------------------------------------------------------------------- factor
// one workgroup per episode: Cholesky factor of A in LDS (left-looking, four threads per row), L back to the workspace,
// alpha = 2 L^-T L^-1 Y, W = Z_S^T alpha
__global__ __launch_bounds__(RIDGE_WG) void ridge_factor_kernel(const float* __restrict__ feats, RidgeShape s, float* __restrict__ A,
                                                                float* __restrict__ alpha, float* __restrict__ W) {
    extern __shared__ float sl[];
    __shared__ double sdiag;
    const int e = blockIdx.x, tid = threadIdx.x, S = s.n_way * s.ns;
    const float* ep = feats + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
    float* Ae = A + (long long)e * S * S;
    for (int idx = tid; idx < S * S; idx += RIDGE_WG) {
        const int i = idx / S, j = idx - i * S;
        if (j <= i) sl[i * (i + 1) / 2 + j] = Ae[idx];
    }
    __syncthreads();
    {
        const int i = tid >> 2, part = tid & 3, rowi = i * (i + 1) / 2;
        for (int k = 0; k < S; ++k) {
            const int rowk = k * (k + 1) / 2;
            const bool live = i >= k && i < S;
            double acc = 0.0;
            if (live)
                for (int j = part; j < k; j += 4) acc += (double)sl[rowi + j] * (double)sl[rowk + j];
            acc = group_sum<4>(acc);
            const double v = live ? (double)sl[rowi + k] - acc : 0.0;
            if (i == k && part == 0) sdiag = (double)(float)sqrt(v);
            __syncthreads();
            if (live && part == 0) sl[rowi + k] = i == k ? (float)sdiag : (float)(v / sdiag);
            __syncthreads();
        }
    }
    for (int idx = tid; idx < S * S; idx += RIDGE_WG) {
        const int i = idx / S, j = idx - i * S;
        if (j <= i) Ae[idx] = sl[i * (i + 1) / 2 + j];
    }
    const int c = tid >> 5, part = tid & 31;
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = (32 * t + part) / s.ns == c ? 2.0 : 0.0;
    solve_lower(sl, S, part, v);
    solve_lower_transposed(sl, S, part, v);
    __syncthreads();                                             // L is dead: the LDS now holds alpha [S][n_way]
    float* ae = alpha + (long long)e * S * s.n_way;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        if (j < S && c < s.n_way) ae[j * s.n_way + c] = sl[j * s.n_way + c] = (float)v[t];
    }
    __syncthreads();
    const int d = tid & (RIDGE_D - 1), c0 = (tid >> 9) * 16;
    double w[16];
    support_combine(ep, s, S, d, c0, sl, w);
    float* We = W + (long long)e * s.n_way * RIDGE_D;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc)
        if (c0 + cc < s.n_way) We[(c0 + cc) * RIDGE_D + d] = (float)w[cc];
}

// ---------------------------------------------------------------------------------------------------------------- scores
// 16 query rows per workgroup, one wave per row; W in LDS in chunks of 16 classes; lane c keeps the row's score of class c
__global__ __launch_bounds__(RIDGE_THREADS) void ridge_scores_kernel(const float* __restrict__ feats, RidgeShape s,
                                                                     const float* __restrict__ W, const float* __restrict__ scale,
                                                                     float* __restrict__ scores, int softmax) {
    __shared__ f32x4 sw[16 * RIDGE_D / 4];
    const int e = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qrows = s.n_way * s.nq;
    const float* ep = feats + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
    const f32x4* We = (const f32x4*)(W + (long long)e * s.n_way * RIDGE_D);
    float* out = scores + (long long)e * qrows * s.n_way;
    const double sc = (double)scale[0];
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
                if (lane == c0 + k) mine[m] = (float)(sc * p);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = blockIdx.x * 16 + wave + 4 * m;
        if (r >= qrows) continue;
        float v = mine[m];
        if (softmax) {
            const float mx = wave_max(lane < s.n_way ? v : -3.4e38f);
            const float ex = lane < s.n_way ? expf(v - mx) : 0.f;
            v = ex / wave_sum(ex);
        }
        if (lane < s.n_way) out[(long long)r * s.n_way + lane] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// query side, one workgroup per (64 columns, episode): dW = scale * Z_Q^T G, the block's share of dscale = sum(W * Z_Q^T G),
// dZ_Q = scale * G W^T
__global__ __launch_bounds__(RIDGE_THREADS) void ridge_bwd_query_kernel(const float* __restrict__ feats, RidgeShape s,
                                                                        const float* __restrict__ W, const float* __restrict__ scale,
                                                                        const float* __restrict__ dscores, int ldg,
                                                                        float* __restrict__ dfeats, int ldd, float* __restrict__ dW,
                                                                        double* __restrict__ dscale_part) {
    __shared__ float sw[RIDGE_MAX_WAY][64];
    __shared__ double sred[RIDGE_THREADS / 64];
    const int e = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = blockIdx.x * 64 + lane;
    const int qrows = s.n_way * s.nq;
    const long long ebase = (long long)e * s.n_way * (s.ns + s.nq);
    const float* ep = feats + ebase * s.ld;
    float* dep = dfeats + ebase * ldd;
    const float* We = W + (long long)e * s.n_way * RIDGE_D;
    float* dWe = dW + (long long)e * s.n_way * RIDGE_D;
    const float* g = dscores + (long long)e * qrows * ldg;
    const double sc = (double)scale[0];
    for (int i = threadIdx.x; i < s.n_way * 64; i += RIDGE_THREADS) sw[i >> 6][i & 63] = We[(i >> 6) * RIDGE_D + blockIdx.x * 64 + (i & 63)];
    double acc[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.0;
    for (int r = 0; r < qrows; ++r) {
        const double z = ep[qry_row(s, r) * s.ld + d];
        const float* gr = g + (long long)r * ldg;
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (wave + 4 * m < s.n_way) acc[m] += z * (double)gr[wave + 4 * m];
    }
    __syncthreads();
    double part = 0.0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int c = wave + 4 * m;
        if (c < s.n_way) {
            part += acc[m] * (double)sw[c][lane];
            dWe[c * RIDGE_D + d] = (float)(sc * acc[m]);
        }
    }
    part = group_sum<64>(part);
    if (lane == 0) sred[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sred[0];
        for (int w = 1; w < RIDGE_THREADS / 64; ++w) t += sred[w];
        dscale_part[e * RIDGE_CB + blockIdx.x] = t;
    }
    for (int r = wave; r < qrows; r += RIDGE_THREADS / 64) {
        const float* gr = g + (long long)r * ldg;
        double a = 0.0;
        for (int c = 0; c < s.n_way; ++c) a += (double)gr[c] * (double)sw[c][lane];
        dep[qry_row(s, r) * ldd + d] = (float)(sc * a);
    }
}

// support side, one workgroup per episode: dalpha = Z_S dW, B = A^-1 dalpha from the saved L,
// dZ_S = alpha (dW - U)^T - B W^T with U[c] = sum_s B[s][c] Z_S[s]; workgroup 0 also sums the dscale shares in order
__global__ __launch_bounds__(RIDGE_WG) void ridge_bwd_support_kernel(const float* __restrict__ feats, RidgeShape s, int episodes,
                                                                     const float* __restrict__ L, const float* __restrict__ alpha,
                                                                     const float* __restrict__ W, const float* __restrict__ dW,
                                                                     const double* __restrict__ dscale_part, float* __restrict__ dfeats,
                                                                     int ldd, float* __restrict__ dscale) {
    extern __shared__ float sl[];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, S = s.n_way * s.ns;
    const long long ebase = (long long)e * s.n_way * (s.ns + s.nq);
    const float* ep = feats + ebase * s.ld;
    float* dep = dfeats + ebase * ldd;
    const float* We = W + (long long)e * s.n_way * RIDGE_D;
    const float* dWe = dW + (long long)e * s.n_way * RIDGE_D;
    if (e == 0 && tid == 0) {
        double t = 0.0;
        for (int i = 0; i < episodes * RIDGE_CB; ++i) t += dscale_part[i];
        dscale[0] = (float)t;
    }
    // dalpha [S][n_way] in LDS as double, one wave per support row
    double* sda = (double*)sl;
    for (int i = wave; i < S; i += RIDGE_WG / 64) {
        const float* x = sup_row(ep, s, i);
        const f32x4 x0 = *(const f32x4*)(x + 4 * lane), x1 = *(const f32x4*)(x + 256 + 4 * lane);
        for (int c = 0; c < s.n_way; ++c) {
            const f32x4* wr = (const f32x4*)(dWe + c * RIDGE_D);
            const double p = group_sum<64>(dot4(x0, wr[lane]) + dot4(x1, wr[64 + lane]));
            if (lane == 0) sda[i * s.n_way + c] = p;
        }
    }
    __syncthreads();
    const int c = tid >> 5, part = tid & 31;
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        v[t] = (j < S && c < s.n_way) ? sda[j * s.n_way + c] : 0.0;
    }
    __syncthreads();
    const float* Le = L + (long long)e * S * S;
    for (int idx = tid; idx < S * S; idx += RIDGE_WG) {
        const int i = idx / S, j = idx - i * S;
        if (j <= i) sl[i * (i + 1) / 2 + j] = Le[idx];
    }
    __syncthreads();
    solve_lower(sl, S, part, v);
    solve_lower_transposed(sl, S, part, v);
    __syncthreads();                                             // L is dead: alpha, B [S][n_way] and dW - U [n_way][D] follow
    float* sa = sl;
    float* sb = sl + S * s.n_way;
    float* sm = sl + 2 * S * s.n_way;
    const float* ae = alpha + (long long)e * S * s.n_way;
    for (int i = tid; i < S * s.n_way; i += RIDGE_WG) sa[i] = ae[i];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        if (j < S && c < s.n_way) sb[j * s.n_way + c] = (float)v[t];
    }
    __syncthreads();
    support_assemble(ep, s, S, tid, sa, sb, sm, We, dWe, dep, ldd);
}

size_t factor_lds(int S, int n_way) {
    const size_t packed = (size_t)S * (S + 1) / 2, coef = (size_t)S * n_way;
    return 4 * (packed > coef ? packed : coef);
}

size_t support_lds(int S, int n_way) {
    const size_t packed = 4 * ((size_t)S * (S + 1) / 2), dal = 8 * (size_t)S * n_way;
    const size_t tail = 4 * (2 * (size_t)S * n_way + (size_t)n_way * RIDGE_D);
    return packed > dal ? (packed > tail ? packed : tail) : (dal > tail ? dal : tail);
}

// the largest dynamic LDS either one-workgroup kernel asks for: the packed triangle at S = 256 (131,584 bytes)
constexpr int RIDGE_MAX_LDS = 4 * (RIDGE_MAX_S * (RIDGE_MAX_S + 1) / 2);
static_assert(4 * (2 * RIDGE_MAX_S * RIDGE_MAX_WAY + RIDGE_MAX_WAY * RIDGE_D) <= RIDGE_MAX_LDS, "support-side tail fits");
static_assert(RIDGE_MAX_LDS <= 160 * 1024, "one CU's LDS");

template <typename K>
int ridge_lds_attr(K kern, MftPerDeviceOnce& once) {
    if (once.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, RIDGE_MAX_LDS);
        if (e != hipSuccess) return (int)e;
        once.mark();
    }
    return 0;
}

}  // namespace

extern "C" int mft_ridge_gram(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                              float lambda_reg, float* A, void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || A == nullptr) return MFT_EINVAL;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    const int tiles = cdiv(n_way * n_support, 32);
    hipLaunchKernelGGL(ridge_gram_kernel, dim3(tiles * tiles, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, feats, s, tiles,
                       lambda_reg, A);
    return mft_launch_status();
}

extern "C" int mft_ridge_factor_solve(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                      float* A, float* alpha, float* W, void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || A == nullptr || alpha == nullptr || W == nullptr)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = ridge_lds_attr(ridge_factor_kernel, once);
    if (rc != 0) return rc;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(ridge_factor_kernel, dim3(episodes), dim3(RIDGE_WG), factor_lds(n_way * n_support, n_way), (hipStream_t)stream,
                       feats, s, A, alpha, W);
    return mft_launch_status();
}

extern "C" int mft_ridge_scores(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                const float* W, const float* scale, float* scores, int softmax, void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || W == nullptr || scale == nullptr || scores == nullptr)
        return MFT_EINVAL;
    if (((uintptr_t)W & 15) != 0) return MFT_EINVAL;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(ridge_scores_kernel, dim3(cdiv((long long)n_way * n_query, 16), episodes), dim3(RIDGE_THREADS), 0,
                       (hipStream_t)stream, feats, s, W, scale, scores, softmax ? 1 : 0);
    return mft_launch_status();
}

extern "C" int mft_ridge_backward_query(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                        const float* W, const float* scale, const float* dscores, int ldg, float* dfeats, int ldd,
                                        float* dW, double* dscale_part, void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || W == nullptr || scale == nullptr || dscores == nullptr ||
        dfeats == nullptr || dW == nullptr || dscale_part == nullptr)
        return MFT_EINVAL;
    if (ldg < n_way || ldd < D) return MFT_EINVAL;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(ridge_bwd_query_kernel, dim3(RIDGE_CB, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, feats, s, W, scale,
                       dscores, ldg, dfeats, ldd, dW, dscale_part);
    return mft_launch_status();
}

extern "C" int mft_ridge_backward_support(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                          const float* L, const float* alpha, const float* W, const float* dW,
                                          const double* dscale_part, float* dfeats, int ldd, float* dscale, void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || L == nullptr || alpha == nullptr || W == nullptr ||
        dW == nullptr || dscale_part == nullptr || dfeats == nullptr || dscale == nullptr)
        return MFT_EINVAL;
    if (ldd < D || ((uintptr_t)dW & 15) != 0) return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = ridge_lds_attr(ridge_bwd_support_kernel, once);
    if (rc != 0) return rc;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(ridge_bwd_support_kernel, dim3(episodes), dim3(RIDGE_WG), support_lds(n_way * n_support, n_way),
                       (hipStream_t)stream, feats, s, episodes, L, alpha, W, dW, dscale_part, dfeats, ldd, dscale);
    return mft_launch_status();
}
