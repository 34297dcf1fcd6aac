// Mahalanobis head: the classifier of Simple CNAPS on pooled features.  Per episode and class c,
//   Q_c = lambda S_c + (1 - lambda) S_t + beta I,  lambda = n / (n + 1),  beta = 1,   scores[q, c] = -1/2 (z_q - mu_c)^T Q_c^-1 (z_q - mu_c)
// with the unbiased class and task covariances S_c, S_t of the support rows.  Q_c and its inverse are never formed: with
// T = Z_S - 1 mu_t^T [S, D], G = T T^T, M_c = a I + b P_c (a = (1 - lambda) / (S - 1), b = lambda / (n - 1), P_c the centring projector
// of class c's rows), K_c = beta M_c^-1 + G (S x S, SPD), d = z_q - mu_c, u = T d, w = K_c^-1 u, r = d - T^T w = beta Q_c^-1 d:
//   scores[q, c] = -(d . r) / (2 beta)      d scores / d d = -r / beta      d scores / d T = w r^T / beta
//
// Forward: mahal_centre_kernel (mu_c, T), mahal_gram_kernel (G), mahal_factor_kernel (one workgroup per (episode, class): K_c and its
// packed Cholesky factor in LDS, then the queries 32 at a time, 32 threads each: u, the two solves, the score from d . r = |d|^2 -
// |L^-1 u|^2; w is kept).
// Backward: every gradient row is a combination of the rows of Z_Q, Mu and T, because r = z_q - mu_c - T^T w:
//   dZ_Q[q] = (-g1[q] z_q + sum_c g[q,c] mu_c + sum_i Om[q,i] T_i) / beta                 g1[q] = sum_c g[q,c]
//   dT[i]   = ( sum_q Om[q,i] z_q - sum_c Ph[c,i] mu_c - sum_j Ps[i,j] T_j) / beta
//   m[c]    = ( sum_q g[q,c] z_q  - gs[c] mu_c         - sum_j Ph[c,j] T_j) / beta         gs[c] = sum_q g[q,c]
//   Om[q,i] = sum_c g[q,c] w_qc[i]     Ph[c,i] = sum_q g[q,c] w_qc[i]     Ps[i,j] = sum_{q,c} g[q,c] w_qc[i] w_qc[j]
//   dZ_S[i] = m[class of i] / n + dT[i] - colmean(dT)
// mahal_coef_kernel (Om, Ph, Ps from g and w), mahal_rows_kernel (the three row products), mahal_support_kernel (the last line).
//
// fp32 storage (G and the three coefficient matrices are float64 work arrays), every sum in double, fixed summation order, no atomics,
// every output element written once; the trip count of every loop is a function of the shape alone and the upstream gradient is
// read from device memory.
#include "ridge_common.h"

namespace {

constexpr double MAHAL_BETA = 1.0;
constexpr int MAHAL_ROWS = 8;                        // output rows per workgroup of mahal_rows_kernel
constexpr int MAHAL_CHUNK = 128;                     // source rows per LDS stage there
constexpr int MAHAL_MAX_LDS = 4 * (RIDGE_MAX_S * (RIDGE_MAX_S + 1) / 2);
static_assert(MAHAL_MAX_LDS + 64 <= 160 * 1024, "one CU's LDS");
static_assert(RIDGE_WG == 32 * 32 && RIDGE_MAX_S == 8 * 32, "a solve takes 32 right-hand sides, 32 threads and 8 rows per thread each");
static_assert(RIDGE_MAX_S <= RIDGE_THREADS && RIDGE_D == 2 * RIDGE_THREADS, "mahal_coef_kernel: a thread per column of Ps; two columns per thread");

__host__ __device__ inline double mahal_lambda(int n) { return (double)n / (double)(n + 1); }

// ---------------------------------------------------------------------------------------------------------------- centre
// a thread per column: the class sums in row order, mu_c, mu_t = (the class sums added in class order) / S, T = z - mu_t
__global__ __launch_bounds__(RIDGE_THREADS) void mahal_centre_kernel(const float* __restrict__ feats, RidgeShape s, float* __restrict__ T,
                                                                     float* __restrict__ Mu) {
    const int e = blockIdx.y, d = blockIdx.x * RIDGE_THREADS + threadIdx.x, C = s.n_way, S = C * s.ns;
    const float* ep = feats + (long long)e * C * (s.ns + s.nq) * s.ld;
    double tot = 0.0;
    for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (int k = 0; k < s.ns; ++k) acc += (double)sup_row(ep, s, c * s.ns + k)[d];
        Mu[((long long)e * C + c) * RIDGE_D + d] = (float)(acc / s.ns);
        tot += acc;
    }
    const double mt = tot / S;
    float* Te = T + (long long)e * S * RIDGE_D;
    for (int i = 0; i < S; ++i) Te[(long long)i * RIDGE_D + d] = (float)((double)sup_row(ep, s, i)[d] - mt);
}

// ---------------------------------------------------------------------------------------------------------------- Gram
// lower triangle of G = T T^T, 32x32 tiles, one tile per workgroup, 2x2 entries per thread (the tiling of dkt_gram_kernel)
__global__ __launch_bounds__(RIDGE_THREADS) void mahal_gram_kernel(const float* __restrict__ T, int S, int tiles, double* __restrict__ G) {
    __shared__ float sa[32][33], sb[32][33];
    const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles;
    if (tj > ti) return;
    const int e = blockIdx.y;
    const float* Te = T + (long long)e * S * RIDGE_D;
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int ia = ti * 32 + lr, ib = tj * 32 + lr;
    const float* pa = ia < S ? Te + (long long)ia * RIDGE_D : nullptr;
    const float* pb = ib < S ? Te + (long long)ib * RIDGE_D : nullptr;
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
    double* Ge = G + (long long)e * S * S;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = ti * 32 + ty + 16 * u, j = tj * 32 + tx + 16 * v;
            if (i < S && j <= i) Ge[(long long)i * S + j] = acc[u][v];
        }
}

// ---------------------------------------------------------------------------------------------------------------- factor and solve
// One workgroup per (class, episode).  K_c = beta M_c^-1 + G with M_c^-1 = (I - P_c) / a + P_c / (a + b) goes into LDS as a packed lower
// triangle and is factored in place.  Then 32 queries at a time, a group of 32 threads per query; thread `part` of a group keeps the
// columns 128 k + 4 part + (0..3), k = 0..3, of d and the rows part (mod 32) of u and w.  S = 1: T = 0, so w = 0 and r = d.
__global__ __launch_bounds__(RIDGE_WG) void mahal_factor_kernel(const float* __restrict__ feats, RidgeShape s, const float* __restrict__ T,
                                                                const float* __restrict__ Mu, const double* __restrict__ G,
                                                                float* __restrict__ scores, float* __restrict__ W) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double sdiag;
    float* sl = (float*)smem;
    const int c = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int group = tid >> 5, part = tid & 31;
    const int C = s.n_way, n = s.ns, S = C * n, Q = C * s.nq;
    const float* ep = feats + (long long)e * C * (s.ns + s.nq) * s.ld;
    const float* Te = T + (long long)e * S * RIDGE_D;
    const float* mu = Mu + ((long long)e * C + c) * RIDGE_D;

    if (S > 1) {
        const double lam = mahal_lambda(n), a = (1.0 - lam) / (S - 1), b = n > 1 ? lam / (n - 1) : 0.0;
        const double off = MAHAL_BETA / a, in = MAHAL_BETA / (a + b) - off;     // M_c^-1 = I / a + (1 / (a + b) - 1 / a) P_c
        const double* Ge = G + (long long)e * S * S;
        const int lo = c * n, hi = lo + n;
        for (int i = wave; i < S; i += RIDGE_WG / 64) {
            const int rowi = i * (i + 1) / 2;
            const bool mine = i >= lo && i < hi;
            for (int j = lane; j <= i; j += 64) {
                double v = Ge[(long long)i * S + j] + (i == j ? off : 0.0);
                if (mine && j >= lo) v += in * ((i == j ? 1.0 : 0.0) - 1.0 / n);
                sl[rowi + j] = (float)v;
            }
        }
        __syncthreads();
        factor_by_size(sl, S, tid, &sdiag);
    }

    for (int q0 = 0; q0 < Q; q0 += 32) {
        const int q = q0 + group;
        const bool live = q < Q;                                  // uniform over the group; a group past the end repeats the last query
        const float* x = ep + qry_row(s, live ? q : Q - 1) * s.ld;
        double d[16], sc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x4 xv = *(const f32x4*)(x + 128 * k + 4 * part), mv = *(const f32x4*)(mu + 128 * k + 4 * part);
#pragma unroll
            for (int xx = 0; xx < 4; ++xx) {
                d[4 * k + xx] = (double)xv[xx] - (double)mv[xx];
                sc += d[4 * k + xx] * d[4 * k + xx];
            }
        }
        double v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = 0.0;
        if (S > 1) {
#pragma unroll
            for (int t = 0; t < 8; ++t)
                for (int kk = 0; kk < 32; ++kk) {
                    const int i = 32 * t + kk;
                    if (i >= S) break;                            // uniform over the workgroup
                    const float* row = Te + (long long)i * RIDGE_D + 4 * part;
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const f32x4 tv = *(const f32x4*)(row + 128 * k);
#pragma unroll
                        for (int xx = 0; xx < 4; ++xx) acc += (double)tv[xx] * d[4 * k + xx];
                    }
                    acc = group_sum<32>(acc);
                    if (part == kk) v[t] = acc;
                }
            solve_lower(sl, S, part, v);
            // d . r = |d|^2 - u . w and u . w = |L^-1 u|^2: both sums are in double, so the difference loses nothing that fp32 storage
            // would keep
#pragma unroll
            for (int t = 0; t < 8; ++t) sc -= v[t] * v[t];
            solve_lower_transposed(sl, S, part, v);
        }
        if (W != nullptr && live) {
            float* wo = W + (((long long)e * Q + q) * C + c) * S;
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (32 * t + part < S) wo[32 * t + part] = (float)v[t];
        }
        sc = group_sum<32>(sc);
        if (live && part == 0) scores[((long long)e * Q + q) * C + c] = (float)(-sc / (2.0 * MAHAL_BETA));
    }
}

// ---------------------------------------------------------------------------------------------------------------- coefficients
// one workgroup per (support row i, episode): Ps[i, :] (a thread per column), Om[:, i], Ph[:, i]; (q, c) pairs in order
__global__ __launch_bounds__(RIDGE_THREADS) void mahal_coef_kernel(RidgeShape s, const float* __restrict__ W, const float* __restrict__ g,
                                                                   double* __restrict__ Om, double* __restrict__ Ph,
                                                                   double* __restrict__ Ps) {
    const int i = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, C = s.n_way, S = C * s.ns, Q = C * s.nq;
    const float* We = W + (long long)e * Q * C * S;
    const float* ge = g + (long long)e * Q * C;
    if (tid < S) {
        double acc = 0.0;
        for (long long qc = 0; qc < (long long)Q * C; ++qc) {
            const double gw = (double)ge[qc] * (double)We[qc * S + i];
            acc += gw * (double)We[qc * S + tid];
        }
        Ps[((long long)e * S + i) * S + tid] = acc;
    }
    for (int q = tid; q < Q; q += RIDGE_THREADS) {
        double acc = 0.0;
        for (int c = 0; c < C; ++c) acc += (double)ge[(long long)q * C + c] * (double)We[((long long)q * C + c) * S + i];
        Om[((long long)e * Q + q) * S + i] = acc;
    }
    if (tid < C) {
        double acc = 0.0;
        for (int q = 0; q < Q; ++q) acc += (double)ge[(long long)q * C + tid] * (double)We[((long long)q * C + tid) * S + i];
        Ph[((long long)e * C + tid) * S + i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- row products
// MAHAL_ROWS output rows per workgroup, two columns per thread.  The workgroups of an episode, in order: the query rows (-> dfeats),
// the rows of dT and the rows of m (-> X [episodes, S + n_way, D]).  A row is a combination of the source rows Z_Q, Mu, T (in this
// order, each in row order); its coefficients are staged in LDS MAHAL_CHUNK sources at a time.
__global__ __launch_bounds__(RIDGE_THREADS) void mahal_rows_kernel(const float* __restrict__ feats, RidgeShape s, const float* __restrict__ T,
                                                                   const float* __restrict__ Mu, const float* __restrict__ g,
                                                                   const double* __restrict__ Om, const double* __restrict__ Ph,
                                                                   const double* __restrict__ Ps, float* __restrict__ X,
                                                                   float* __restrict__ dfeats, int ldd) {
    __shared__ double sc[MAHAL_ROWS][MAHAL_CHUNK];
    const int e = blockIdx.y, tid = threadIdx.x, C = s.n_way, S = C * s.ns, Q = C * s.nq;
    const int qb = (Q + MAHAL_ROWS - 1) / MAHAL_ROWS, tb = (S + MAHAL_ROWS - 1) / MAHAL_ROWS;
    const int kind = (int)blockIdx.x < qb ? 0 : ((int)blockIdx.x < qb + tb ? 1 : 2);       // 0: dZ_Q, 1: dT, 2: m
    const int r0 = ((int)blockIdx.x - (kind == 0 ? 0 : (kind == 1 ? qb : qb + tb))) * MAHAL_ROWS;
    const int rows = kind == 0 ? Q : (kind == 1 ? S : C);
    const long long row0 = (long long)e * C * (s.ns + s.nq);
    const float* ep = feats + row0 * s.ld;
    const float* Te = T + (long long)e * S * RIDGE_D;
    const float* Me = Mu + (long long)e * C * RIDGE_D;
    const float* ge = g + (long long)e * Q * C;
    const double* Ome = Om + (long long)e * Q * S;
    const double* Phe = Ph + (long long)e * C * S;
    const double* Pse = Ps + (long long)e * S * S;

    double acc[MAHAL_ROWS][2];
#pragma unroll
    for (int r = 0; r < MAHAL_ROWS; ++r) acc[r][0] = acc[r][1] = 0.0;
    for (int seg = kind == 0 ? 1 : 0; seg < 3; ++seg) {            // the sources: 0 = Z_Q, 1 = Mu, 2 = T
        const int len = seg == 0 ? Q : (seg == 1 ? C : S);
        for (int l0 = 0; l0 < len; l0 += MAHAL_CHUNK) {
            __syncthreads();
            for (int idx = tid; idx < MAHAL_ROWS * MAHAL_CHUNK; idx += RIDGE_THREADS) {
                const int r = idx / MAHAL_CHUNK, l = l0 + (idx - r * MAHAL_CHUNK), row = r0 + r;
                double v = 0.0;
                if (row < rows && l < len) {
                    if (kind == 0) {
                        v = seg == 1 ? (double)ge[(long long)row * C + l] : Ome[(long long)row * S + l];
                    } else if (kind == 1) {
                        v = seg == 0 ? Ome[(long long)l * S + row] : (seg == 1 ? -Phe[(long long)l * S + row] : -Pse[(long long)row * S + l]);
                    } else if (seg == 0) {
                        v = (double)ge[(long long)l * C + row];
                    } else if (seg == 2) {
                        v = -Phe[(long long)row * S + l];
                    } else if (l == row) {
                        double gs = 0.0;
                        for (int q = 0; q < Q; ++q) gs += (double)ge[(long long)q * C + row];
                        v = -gs;
                    }
                }
                sc[r][idx - r * MAHAL_CHUNK] = v;
            }
            __syncthreads();
            const int cnt = min(MAHAL_CHUNK, len - l0);
            for (int l = 0; l < cnt; ++l) {
                const float* src = seg == 0 ? ep + qry_row(s, l0 + l) * s.ld : (seg == 1 ? Me : Te) + (long long)(l0 + l) * RIDGE_D;
                const double v0 = src[tid], v1 = src[RIDGE_THREADS + tid];
#pragma unroll
                for (int r = 0; r < MAHAL_ROWS; ++r) {
                    acc[r][0] += sc[r][l] * v0;
                    acc[r][1] += sc[r][l] * v1;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < MAHAL_ROWS; ++r) {
        const int row = r0 + r;
        if (row >= rows) continue;
        float* o;
        if (kind == 0) {
            double g1 = 0.0;
            for (int c = 0; c < C; ++c) g1 += (double)ge[(long long)row * C + c];
            const float* x = ep + qry_row(s, row) * s.ld;
            acc[r][0] -= g1 * (double)x[tid];
            acc[r][1] -= g1 * (double)x[RIDGE_THREADS + tid];
            o = dfeats + (row0 + qry_row(s, row)) * ldd;
        } else {
            o = X + ((long long)e * (S + C) + (kind == 1 ? row : S + row)) * RIDGE_D;
        }
        o[tid] = (float)(acc[r][0] / MAHAL_BETA);
        o[RIDGE_THREADS + tid] = (float)(acc[r][1] / MAHAL_BETA);
    }
}

// ---------------------------------------------------------------------------------------------------------------- support rows
// a thread per column: dZ_S[i] = m[class of i] / n + dT[i] - colmean(dT), the column mean added in row order
__global__ __launch_bounds__(RIDGE_THREADS) void mahal_support_kernel(RidgeShape s, const float* __restrict__ X, float* __restrict__ dfeats,
                                                                      int ldd) {
    const int e = blockIdx.y, d = blockIdx.x * RIDGE_THREADS + threadIdx.x, C = s.n_way, S = C * s.ns;
    const float* Xe = X + (long long)e * (S + C) * RIDGE_D;
    float* de = dfeats + (long long)e * C * (s.ns + s.nq) * ldd;
    double tot = 0.0;
    for (int i = 0; i < S; ++i) tot += (double)Xe[(long long)i * RIDGE_D + d];
    const double mean = tot / S;
    for (int i = 0; i < S; ++i) {
        const int c = i / s.ns;
        const double v = (double)Xe[(long long)(S + c) * RIDGE_D + d] / s.ns + (double)Xe[(long long)i * RIDGE_D + d] - mean;
        de[(long long)(c * (s.ns + s.nq) + (i - c * s.ns)) * ldd + d] = (float)v;
    }
}

inline bool mahal_ok(int episodes, int n_way, int n_support, int n_query, int D) {
    if (episodes < 1 || episodes > 65535 || n_way < 1 || n_way > RIDGE_MAX_WAY || n_support < 1 || n_query < 1 || D != RIDGE_D) return false;
    if ((long long)n_way * n_support > RIDGE_MAX_S) return false;
    return (long long)episodes * n_way * ((long long)n_support + n_query) < (1ll << 31) / RIDGE_D;
}

inline bool mahal_rows_ok(const void* p, int ld) { return p != nullptr && ((uintptr_t)p & 15) == 0 && ld >= RIDGE_D && (ld & 3) == 0; }

}  // namespace

extern "C" int mft_mahalanobis_centre(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, float* T,
                                      float* Mu, void* stream) {
    if (!mahal_ok(episodes, n_way, n_support, n_query, D) || !mahal_rows_ok(feats, ld) || !mahal_rows_ok(T, D) || !mahal_rows_ok(Mu, D))
        return MFT_EINVAL;
    const RidgeShape s{n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(mahal_centre_kernel, dim3(RIDGE_D / RIDGE_THREADS, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, feats, s, T,
                       Mu);
    return mft_launch_status();
}

extern "C" int mft_mahalanobis_gram(int episodes, int n_way, int n_support, int n_query, int D, const float* T, double* G, void* stream) {
    if (!mahal_ok(episodes, n_way, n_support, n_query, D) || !mahal_rows_ok(T, D) || G == nullptr) return MFT_EINVAL;
    const int S = n_way * n_support, tiles = cdiv(S, 32);
    hipLaunchKernelGGL(mahal_gram_kernel, dim3(tiles * tiles, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, T, S, tiles, G);
    return mft_launch_status();
}

extern "C" int mft_mahalanobis_scores(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                      const float* T, const float* Mu, const double* G, float* scores, float* W, void* stream) {
    if (!mahal_ok(episodes, n_way, n_support, n_query, D) || !mahal_rows_ok(feats, ld) || !mahal_rows_ok(T, D) || !mahal_rows_ok(Mu, D) ||
        G == nullptr || scores == nullptr)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    if (once.need()) {
        hipError_t err = hipFuncSetAttribute((const void*)mahal_factor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MAHAL_MAX_LDS);
        if (err != hipSuccess) return (int)err;
        once.mark();
    }
    const RidgeShape s{n_way, n_support, n_query, ld};
    const int S = n_way * n_support;
    hipLaunchKernelGGL(mahal_factor_kernel, dim3(n_way, episodes), dim3(RIDGE_WG), 4 * ((size_t)S * (S + 1) / 2), (hipStream_t)stream, feats,
                       s, T, Mu, G, scores, W);
    return mft_launch_status();
}

extern "C" int mft_mahalanobis_coef(int episodes, int n_way, int n_support, int n_query, int D, const float* W, const float* dscores,
                                    double* Om, double* Ph, double* Ps, void* stream) {
    if (!mahal_ok(episodes, n_way, n_support, n_query, D) || W == nullptr || dscores == nullptr || Om == nullptr || Ph == nullptr ||
        Ps == nullptr)
        return MFT_EINVAL;
    const RidgeShape s{n_way, n_support, n_query, RIDGE_D};
    hipLaunchKernelGGL(mahal_coef_kernel, dim3(n_way * n_support, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, s, W, dscores, Om,
                       Ph, Ps);
    return mft_launch_status();
}

extern "C" int mft_mahalanobis_backward(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                        const float* T, const float* Mu, const float* dscores, const double* Om, const double* Ph,
                                        const double* Ps, float* X, float* dfeats, int ldd, void* stream) {
    if (!mahal_ok(episodes, n_way, n_support, n_query, D) || !mahal_rows_ok(feats, ld) || !mahal_rows_ok(T, D) || !mahal_rows_ok(Mu, D) ||
        dscores == nullptr || Om == nullptr || Ph == nullptr || Ps == nullptr || !mahal_rows_ok(X, D) || !mahal_rows_ok(dfeats, ldd))
        return MFT_EINVAL;
    const RidgeShape s{n_way, n_support, n_query, ld};
    const int S = n_way * n_support, Q = n_way * n_query;
    hipLaunchKernelGGL(mahal_rows_kernel, dim3(cdiv(Q, MAHAL_ROWS) + cdiv(S, MAHAL_ROWS) + cdiv(n_way, MAHAL_ROWS), episodes),
                       dim3(RIDGE_THREADS), 0, (hipStream_t)stream, feats, s, T, Mu, dscores, Om, Ph, Ps, X, dfeats, ldd);
    const int st = mft_launch_status();
    if (st != 0) return st;
    hipLaunchKernelGGL(mahal_support_kernel, dim3(RIDGE_D / RIDGE_THREADS, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, s, X, dfeats,
                       ldd);
    return mft_launch_status();
}
