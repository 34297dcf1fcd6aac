// Deep Kernel Transfer head: a Gaussian process on the backbone's features, trained through its marginal
// likelihood and scored with its posterior mean, every episode of a step per launch.
//
//   u = z / max(|z|, 1e-12) (cossim) or z / sqrt(D) (linear)    s = softplus(raw_outputscale)    noise = 1e-4 + softplus(raw_noise)
//   K = s U U^T + noise I    R = Y - mean (Y = +1 on the row's class, -1 elsewhere)    A = K^-1 R
//   loss   = (tr(R^T A) / 2 + n_way log det K / 2 + n_way M log(2 pi) / 2) / M     on all M = N rows of the episode
//   scores = mean + U_Q W,  W = s U_S^T A_S                                         on the M = S support rows
//
// Layout: feats as for csrc/ridge.hip ([episodes, n_way, n_support + n_query, D = 512], row stride ld).  U [rows, D] and nrm [rows]
// (float64, |z|) are in the row order of feats.  The POINTS of a launch are the rows the process conditions on: every row of the
// episode in row order for the loss (the kernels then see the shape {n_way, n_support + n_query, 0}), the support rows class-major
// for the scores.  K [episodes, M, M] (lower triangle only), L [episodes, M (M + 1) / 2] (packed, row after row),
// A [episodes, M, n_way], V = K^-1 U [episodes, M, D], B = A^T U and W [episodes, n_way, D].
//
// Storage is fp32; every sum, the logarithms, the factor's pivots and both triangular solves run in double inside the kernels and
// round once on the store.  No atomics; every sum runs in a fixed order, so two launches on the same input are bit-identical and
// an episode's result does not depend on the episodes beside it.  No kernel waits for another workgroup and the trip count of
// every loop is a function of the shape arguments alone; the three hyperparameters and the upstream gradient are read from device
// memory, so a captured step replays with their current values.
#include "ridge_common.h"

namespace {

constexpr int DKT_MAX_M = 256;                      // points of one episode: the packed factor is kept in one workgroup's LDS
constexpr int DKT_COLS = 32;                        // right-hand sides per workgroup of the V solve
constexpr int DKT_STATS = 4;                        // per episode: loss, sum A, sum A^2, log det K
constexpr double DKT_NORM_EPS = 1e-12;
constexpr double DKT_NOISE_FLOOR = 1e-4;
constexpr double DKT_LOG_2PI = 1.8378770664093453;
static_assert(RIDGE_WG == 32 * DKT_COLS && RIDGE_MAX_WAY <= DKT_COLS, "a solve takes 32 columns, 32 threads each");
static_assert(RIDGE_THREADS / 64 == 4, "dkt_grad_kernel and dkt_hyper_kernel add four partial sums");

__device__ __forceinline__ double softplus_d(double x) { return (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }

// ---------------------------------------------------------------------------------------------------------------- normalise
// one wave per feats row: nrm = |z|, u = z / max(nrm, 1e-12) or z / sqrt(D)
__global__ __launch_bounds__(RIDGE_THREADS) void dkt_normalise_kernel(const float* __restrict__ feats, int ld, long long rows, int linear,
                                                                      float* __restrict__ U, double* __restrict__ nrm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * (RIDGE_THREADS / 64) + wave;
    if (g >= rows) return;                                       // uniform over the wave
    const float* x = feats + g * ld;
    const f32x4 x0 = *(const f32x4*)(x + 4 * lane), x1 = *(const f32x4*)(x + 256 + 4 * lane);
    const double n = sqrt(group_sum<64>(dot4(x0, x0) + dot4(x1, x1)));
    const double div = linear ? sqrt((double)RIDGE_D) : (n > DKT_NORM_EPS ? n : DKT_NORM_EPS);
    if (lane == 0) nrm[g] = n;
    f32x4 o0, o1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o0[q] = (float)((double)x0[q] / div);
        o1[q] = (float)((double)x1[q] / div);
    }
    float* ur = U + g * RIDGE_D;
    *(f32x4*)(ur + 4 * lane) = o0;
    *(f32x4*)(ur + 256 + 4 * lane) = o1;
}

// ---------------------------------------------------------------------------------------------------------------- Gram
// lower triangle of K = s U_P U_P^T + noise I over the launch's points, 32x32 tiles, one tile per workgroup, 2x2 entries per thread
__global__ __launch_bounds__(RIDGE_THREADS) void dkt_gram_kernel(const float* __restrict__ U, RidgeShape s, int tiles,
                                                                 const float* __restrict__ raw_os, const float* __restrict__ raw_noise,
                                                                 float* __restrict__ K) {
    __shared__ float sa[32][33], sb[32][33];
    const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles;
    if (tj > ti) return;
    const int e = blockIdx.y, M = s.n_way * s.ns;
    const float* ep = U + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int ia = ti * 32 + lr, ib = tj * 32 + lr;
    const float* pa = ia < M ? sup_row(ep, s, ia) : nullptr;
    const float* pb = ib < M ? sup_row(ep, s, ib) : nullptr;
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
    const double scale = softplus_d((double)raw_os[0]), noise = DKT_NOISE_FLOOR + softplus_d((double)raw_noise[0]);
    float* Ke = K + (long long)e * M * M;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = ti * 32 + ty + 16 * u, j = tj * 32 + tx + 16 * v;
            if (i < M && j <= i) Ke[(long long)i * M + j] = (float)(scale * acc[u][v] + (i == j ? noise : 0.0));
        }
}

// ---------------------------------------------------------------------------------------------------------------- factor
// one workgroup per episode: Cholesky factor of K in LDS, A = K^-1 (Y - mean) by the two solves; then either the episode's loss
// from the factor's diagonal and tr(R^T A) (stats != NULL) or W = s U_P^T A (W != NULL)
__global__ __launch_bounds__(RIDGE_WG) void dkt_factor_kernel(const float* __restrict__ U, RidgeShape s, const float* __restrict__ K,
                                                              const float* __restrict__ mean, const float* __restrict__ raw_os,
                                                              float* __restrict__ L, float* __restrict__ A, double* __restrict__ stats,
                                                              float* __restrict__ W) {
    extern __shared__ float sl[];
    __shared__ double sdiag;
    __shared__ double sred[DKT_STATS][RIDGE_WG / 64];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, M = s.n_way * s.ns;
    const float* Ke = K + (long long)e * M * M;
    for (int idx = tid; idx < M * M; idx += RIDGE_WG) {
        const int i = idx / M, j = idx - i * M;
        if (j <= i) sl[i * (i + 1) / 2 + j] = Ke[idx];
    }
    __syncthreads();
    factor_by_size(sl, M, tid, &sdiag);
    const int packed = M * (M + 1) / 2;
    if (L) {
        float* Le = L + (long long)e * packed;
        for (int idx = tid; idx < packed; idx += RIDGE_WG) Le[idx] = sl[idx];
    }
    const double logd = tid < M ? log((double)sl[tid * (tid + 1) / 2 + tid]) : 0.0;
    const int c = tid >> 5, part = tid & 31;
    const double mu = (double)mean[0];
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        v[t] = (j < M && c < s.n_way) ? (j / s.ns == c ? 1.0 : -1.0) - mu : 0.0;
    }
    solve_lower(sl, M, part, v);
    solve_lower_transposed(sl, M, part, v);
    __syncthreads();                                             // L is dead: the LDS now holds A [M][n_way]
    float* Ae = A + (long long)e * M * s.n_way;
    double quad = 0.0, sum1 = 0.0, sum2 = 0.0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        if (j < M && c < s.n_way) {
            const float a = (float)v[t];
            Ae[j * s.n_way + c] = sl[j * s.n_way + c] = a;
            quad += ((j / s.ns == c ? 1.0 : -1.0) - mu) * v[t];
            sum1 += (double)a;
            sum2 += (double)a * (double)a;
        }
    }
    if (stats) {
        const double r[DKT_STATS] = {group_sum<64>(quad), group_sum<64>(sum1), group_sum<64>(sum2), group_sum<64>(logd)};
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < DKT_STATS; ++q) sred[q][wave] = r[q];
        }
    }
    __syncthreads();
    if (stats && tid == 0) {
        double t[DKT_STATS];
#pragma unroll
        for (int q = 0; q < DKT_STATS; ++q) {
            t[q] = sred[q][0];
            for (int w = 1; w < RIDGE_WG / 64; ++w) t[q] += sred[q][w];
        }
        const double logdet = 2.0 * t[3], C = s.n_way;
        double* st = stats + (long long)e * DKT_STATS;
        st[0] = (0.5 * t[0] + 0.5 * C * logdet + 0.5 * C * M * DKT_LOG_2PI) / M;
        st[1] = t[1];
        st[2] = t[2];
        st[3] = logdet;
    }
    if (W) {
        const float* ep = U + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
        const int d = tid & (RIDGE_D - 1), c0 = (tid >> 9) * 16;
        double w[16];
        support_combine(ep, s, M, d, c0, sl, w);
        const double scale = softplus_d((double)raw_os[0]);
        float* We = W + (long long)e * s.n_way * RIDGE_D;
#pragma unroll
        for (int cc = 0; cc < 16; ++cc)
            if (c0 + cc < s.n_way) We[(c0 + cc) * RIDGE_D + d] = (float)(scale * w[cc]);
    }
}

// the step's loss = the mean of the episodes' losses, added in episode order; *loss_sum (nullable) += it
__global__ void dkt_loss_mean_kernel(const double* __restrict__ stats, int episodes, float* __restrict__ loss,
                                     double* __restrict__ loss_sum) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double t = 0.0;
    for (int e = 0; e < episodes; ++e) t += stats[(long long)e * DKT_STATS];
    t /= (double)episodes;
    loss[0] = (float)t;
    if (loss_sum) *loss_sum += (double)(float)t;                  // the stored loss: what the eager loop's loss.item() adds
}

// ---------------------------------------------------------------------------------------------------------------- backward
// one workgroup per (32 columns of U, episode): V = K^-1 U for those columns from the saved factor, the same columns of
// B = A^T U (thread (c, x): class c, column x of the block), and the block's share of tr K^-1 = |L^-1|_F^2 from a forward solve of
// the unit vectors 32 b .. 32 b + 31 (a sum of squares: N - s sum <u_i, V_i> gives the same trace times the noise, but cancels)
__global__ __launch_bounds__(RIDGE_WG) void dkt_solve_kernel(const float* __restrict__ U, int M, int n_way, const float* __restrict__ L,
                                                             const float* __restrict__ A, float* __restrict__ V, float* __restrict__ B,
                                                             double* __restrict__ trace) {
    extern __shared__ float sl[];
    __shared__ double sred[RIDGE_WG / 64];
    const int e = blockIdx.y, tid = threadIdx.x, col0 = blockIdx.x * DKT_COLS;
    const int packed = M * (M + 1) / 2;
    const float* Le = L + (long long)e * packed;
    for (int idx = tid; idx < packed; idx += RIDGE_WG) sl[idx] = Le[idx];
    const float* Ue = U + (long long)e * M * RIDGE_D;
    const int c = tid >> 5, part = tid & 31;
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        v[t] = j < M ? (double)Ue[(long long)j * RIDGE_D + col0 + c] : 0.0;
    }
    __syncthreads();
    solve_lower(sl, M, part, v);
    solve_lower_transposed(sl, M, part, v);
    float* Ve = V + (long long)e * M * RIDGE_D;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        if (j < M) Ve[(long long)j * RIDGE_D + col0 + c] = (float)v[t];
    }
    if (c < n_way) {
        const float* Ae = A + (long long)e * M * n_way;
        double acc = 0.0;
        for (int i = 0; i < M; ++i) acc += (double)Ae[i * n_way + c] * (double)Ue[(long long)i * RIDGE_D + col0 + part];
        B[((long long)e * n_way + c) * RIDGE_D + col0 + part] = (float)acc;
    }
    double sq = 0.0;
    if (col0 < M) {                                              // uniform over the workgroup
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = (32 * t + part == col0 + c && col0 + c < M) ? 1.0 : 0.0;
        solve_lower(sl, M, part, v);
#pragma unroll
        for (int t = 0; t < 8; ++t) sq += v[t] * v[t];
    }
    sq = group_sum<64>(sq);
    if ((tid & 63) == 0) sred[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
        double t = sred[0];
        for (int w = 1; w < RIDGE_WG / 64; ++w) t += sred[w];
        trace[(long long)e * (RIDGE_D / DKT_COLS) + blockIdx.x] = t;
    }
}

// four rows per workgroup, two columns per thread: (G U)_i = (n_way V_i - sum_c A_ic B_c) / (2 M), dU_i = 2 s g (G U)_i, then through
// the normalisation: dz = (dU - u <u, dU>) / |z| (cossim, |z| >= 1e-12), dU / 1e-12 (cossim below it), dU / sqrt(D) (linear);
// part [rows] = <(G U)_i, u_i>, the row's share of the outputscale gradient
__global__ __launch_bounds__(RIDGE_THREADS) void dkt_grad_kernel(const float* __restrict__ U, const double* __restrict__ nrm, int M,
                                                                 int n_way, int episodes, int linear, const float* __restrict__ A,
                                                                 const float* __restrict__ V, const float* __restrict__ B,
                                                                 const float* __restrict__ raw_os, const float* __restrict__ gout,
                                                                 float* __restrict__ dfeats, int ldd, double* __restrict__ part) {
    __shared__ double sred[4][RIDGE_THREADS / 64];
    const int e = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i0 = blockIdx.x * 4;
    const int d0 = tid, d1 = tid + RIDGE_THREADS;
    const float* Ae = A + (long long)e * M * n_way;
    const float* Be = B + (long long)e * n_way * RIDGE_D;
    double ui[4][2], vi[4][2], gu[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool live = i0 + q < M;
        const long long g = (long long)e * M + i0 + q;
        ui[q][0] = live ? (double)U[g * RIDGE_D + d0] : 0.0;
        ui[q][1] = live ? (double)U[g * RIDGE_D + d1] : 0.0;
        vi[q][0] = live ? (double)V[g * RIDGE_D + d0] : 0.0;
        vi[q][1] = live ? (double)V[g * RIDGE_D + d1] : 0.0;
        gu[q][0] = gu[q][1] = 0.0;
    }
    for (int c = 0; c < n_way; ++c) {
        const double b0 = Be[c * RIDGE_D + d0], b1 = Be[c * RIDGE_D + d1];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double a = i0 + q < M ? (double)Ae[(i0 + q) * n_way + c] : 0.0;
            gu[q][0] += a * b0;
            gu[q][1] += a * b1;
        }
    }
    const double inv2m = 0.5 / (double)M;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        gu[q][0] = ((double)n_way * vi[q][0] - gu[q][0]) * inv2m;
        gu[q][1] = ((double)n_way * vi[q][1] - gu[q][1]) * inv2m;
        const double p = group_sum<64>(gu[q][0] * ui[q][0] + gu[q][1] * ui[q][1]);
        if (lane == 0) sred[q][wave] = p;
    }
    __syncthreads();
    const double coef = 2.0 * softplus_d((double)raw_os[0]) * (gout ? (double)gout[0] : 1.0) / (double)episodes;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (i0 + q >= M) continue;                               // uniform over the workgroup
        const long long g = (long long)e * M + i0 + q;
        const double p = ((sred[q][0] + sred[q][1]) + sred[q][2]) + sred[q][3];
        if (tid == 0) part[g] = p;
        double z0 = coef * gu[q][0], z1 = coef * gu[q][1];
        if (linear) {
            const double r = 1.0 / sqrt((double)RIDGE_D);
            z0 *= r;
            z1 *= r;
        } else {
            const double n = nrm[g];
            if (n >= DKT_NORM_EPS) {
                const double t = coef * p;                       // <u, dU>
                z0 = (z0 - ui[q][0] * t) / n;
                z1 = (z1 - ui[q][1] * t) / n;
            } else {
                z0 /= DKT_NORM_EPS;
                z1 /= DKT_NORM_EPS;
            }
        }
        dfeats[g * ldd + d0] = (float)z0;
        dfeats[g * ldd + d1] = (float)z1;
    }
}

// one workgroup: the three scalar gradients, the episodes' shares added in episode order, each episode's rows in a fixed order.
// With G = (n_way K^-1 - A A^T) / (2 M):  sum_ij G_ij <u_i, u_j> = sum_i <(G U)_i, u_i>,  tr K^-1 = the sum of the solve launch's shares,
// tr G = (n_way tr K^-1 - sum A^2) / (2 M);  (dmean, draw_os, draw_noise) = g / episodes * (-sum A / M, sigmoid(raw_os) sum G_ij <u_i, u_j>,
// sigmoid(raw_noise) tr G)
__global__ __launch_bounds__(RIDGE_THREADS) void dkt_hyper_kernel(const double* __restrict__ part, const double* __restrict__ trace,
                                                                  const double* __restrict__ stats, int M,
                                                                  int n_way, int episodes, const float* __restrict__ raw_os,
                                                                  const float* __restrict__ raw_noise, const float* __restrict__ gout,
                                                                  float* __restrict__ dmean_out, float* __restrict__ dos_out,
                                                                  float* __restrict__ dnoise_out) {
    __shared__ double sred[RIDGE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double dmean = 0.0, dos = 0.0, dnoise = 0.0;
    for (int e = 0; e < episodes; ++e) {
        const double p = group_sum<64>(tid < M ? part[(long long)e * M + tid] : 0.0);
        __syncthreads();
        if (lane == 0) sred[wave] = p;
        __syncthreads();
        const double sp = ((sred[0] + sred[1]) + sred[2]) + sred[3];
        const double* st = stats + (long long)e * DKT_STATS;
        double trkinv = 0.0;
        for (int b = 0; b < RIDGE_D / DKT_COLS; ++b) trkinv += trace[(long long)e * (RIDGE_D / DKT_COLS) + b];
        dmean += -st[1] / (double)M;
        dos += sp;
        dnoise += ((double)n_way * trkinv - st[2]) * (0.5 / (double)M);
    }
    if (tid == 0) {
        const double g = (gout ? (double)gout[0] : 1.0) / (double)episodes;
        dmean_out[0] = (float)(g * dmean);
        dos_out[0] = (float)(g * sigmoid_d((double)raw_os[0]) * dos);
        dnoise_out[0] = (float)(g * sigmoid_d((double)raw_noise[0]) * dnoise);
    }
}

// ---------------------------------------------------------------------------------------------------------------- scores
// 16 query rows per workgroup, one wave per row; W in LDS in chunks of 16 classes; lane c keeps the row's score of class c
__global__ __launch_bounds__(RIDGE_THREADS) void dkt_scores_kernel(const float* __restrict__ U, RidgeShape s, const float* __restrict__ W,
                                                                   const float* __restrict__ mean, float* __restrict__ scores) {
    __shared__ f32x4 sw[16 * RIDGE_D / 4];
    const int e = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qrows = s.n_way * s.nq;
    const float* ep = U + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
    const f32x4* We = (const f32x4*)(W + (long long)e * s.n_way * RIDGE_D);
    float* out = scores + (long long)e * qrows * s.n_way;
    const double mu = (double)mean[0];
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
                if (lane == c0 + k) mine[m] = (float)(mu + p);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = blockIdx.x * 16 + wave + 4 * m;
        if (r < qrows && lane < s.n_way) out[(long long)r * s.n_way + lane] = mine[m];
    }
}

// the points of a launch as a RidgeShape over U (row stride D): every row of the episode (loss), or the support rows (scores)
inline RidgeShape dkt_points(int n_way, int n_support, int n_query, int support_only) {
    return support_only ? RidgeShape{n_way, n_support, n_query, RIDGE_D} : RidgeShape{n_way, n_support + n_query, 0, RIDGE_D};
}

inline bool dkt_shape_ok(int episodes, int n_way, int n_support, int n_query, int D, int support_only) {
    if (episodes < 1 || n_way < 1 || n_way > RIDGE_MAX_WAY || n_support < 1 || n_query < 1 || D != RIDGE_D) return false;
    if ((long long)n_way * ((long long)n_support + (support_only ? 0 : n_query)) > DKT_MAX_M) return false;
    return (long long)episodes * n_way * ((long long)n_support + n_query) < (1ll << 31) / RIDGE_D;
}

inline bool dkt_rows_ok(const void* p, int ld) { return p != nullptr && ld >= RIDGE_D && (ld & 3) == 0 && ((uintptr_t)p & 15) == 0; }

// the largest dynamic LDS either one-workgroup kernel asks for: the packed triangle at M = 256 (131,584 bytes); beside it the
// factor kernel keeps 520 bytes of static LDS
constexpr int DKT_MAX_LDS = 4 * (DKT_MAX_M * (DKT_MAX_M + 1) / 2);
static_assert(DKT_MAX_LDS + 8 + 8 * DKT_STATS * (RIDGE_WG / 64) <= 160 * 1024, "one CU's LDS");
static_assert(4 * DKT_MAX_M * RIDGE_MAX_WAY <= DKT_MAX_LDS, "A [M][n_way] fits where the factor was");

size_t dkt_factor_lds(int M, int n_way) {
    const size_t packed = (size_t)M * (M + 1) / 2, coef = (size_t)M * n_way;
    return 4 * (packed > coef ? packed : coef);
}

template <typename K>
int dkt_lds_attr(K kern, MftPerDeviceOnce& once) {
    if (once.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, DKT_MAX_LDS);
        if (e != hipSuccess) return (int)e;
        once.mark();
    }
    return 0;
}

}  // namespace

extern "C" int mft_dkt_normalise(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, int linear,
                                 float* U, double* nrm, void* stream) {
    if (!dkt_shape_ok(episodes, n_way, n_support, n_query, D, 1) || !dkt_rows_ok(feats, ld) || !dkt_rows_ok(U, D) || nrm == nullptr)
        return MFT_EINVAL;
    const long long rows = (long long)episodes * n_way * (n_support + n_query);
    hipLaunchKernelGGL(dkt_normalise_kernel, dim3((unsigned)cdiv(rows, RIDGE_THREADS / 64)), dim3(RIDGE_THREADS), 0, (hipStream_t)stream,
                       feats, ld, rows, linear ? 1 : 0, U, nrm);
    return mft_launch_status();
}

extern "C" int mft_dkt_gram(int episodes, int n_way, int n_support, int n_query, int D, int support_only, const float* U,
                            const float* raw_outputscale, const float* raw_noise, float* K, void* stream) {
    if (!dkt_shape_ok(episodes, n_way, n_support, n_query, D, support_only) || !dkt_rows_ok(U, D) || raw_outputscale == nullptr ||
        raw_noise == nullptr || K == nullptr)
        return MFT_EINVAL;
    const RidgeShape s = dkt_points(n_way, n_support, n_query, support_only);
    const int tiles = cdiv(s.n_way * s.ns, 32);
    hipLaunchKernelGGL(dkt_gram_kernel, dim3(tiles * tiles, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, U, s, tiles,
                       raw_outputscale, raw_noise, K);
    return mft_launch_status();
}

extern "C" int mft_dkt_factor(int episodes, int n_way, int n_support, int n_query, int D, int support_only, const float* U,
                              const float* K, const float* mean, const float* raw_outputscale, float* L, float* A, double* stats,
                              float* loss, double* loss_sum, float* W, void* stream) {
    if (!dkt_shape_ok(episodes, n_way, n_support, n_query, D, support_only) || !dkt_rows_ok(U, D) || K == nullptr || mean == nullptr ||
        raw_outputscale == nullptr || A == nullptr)
        return MFT_EINVAL;
    // the loss launch reduces (stats and loss, no W); the scores launch combines (W, no stats)
    if (support_only ? (W == nullptr || stats != nullptr || loss != nullptr) : (W != nullptr || stats == nullptr || loss == nullptr))
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = dkt_lds_attr(dkt_factor_kernel, once);
    if (rc != 0) return rc;
    const RidgeShape s = dkt_points(n_way, n_support, n_query, support_only);
    hipLaunchKernelGGL(dkt_factor_kernel, dim3(episodes), dim3(RIDGE_WG), dkt_factor_lds(s.n_way * s.ns, n_way), (hipStream_t)stream, U, s,
                       K, mean, raw_outputscale, L, A, stats, W);
    if (stats != nullptr) {
        const int st = mft_launch_status();
        if (st != 0) return st;
        hipLaunchKernelGGL(dkt_loss_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, episodes, loss, loss_sum);
    }
    return mft_launch_status();
}

extern "C" int mft_dkt_solve(int episodes, int n_way, int n_support, int n_query, int D, const float* U, const float* L, const float* A,
                             float* V, float* B, double* trace, void* stream) {
    if (!dkt_shape_ok(episodes, n_way, n_support, n_query, D, 0) || U == nullptr || L == nullptr || A == nullptr || V == nullptr ||
        B == nullptr || trace == nullptr)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = dkt_lds_attr(dkt_solve_kernel, once);
    if (rc != 0) return rc;
    const int M = n_way * (n_support + n_query);
    hipLaunchKernelGGL(dkt_solve_kernel, dim3(RIDGE_D / DKT_COLS, episodes), dim3(RIDGE_WG), 4 * ((size_t)M * (M + 1) / 2),
                       (hipStream_t)stream, U, M, n_way, L, A, V, B, trace);
    return mft_launch_status();
}

extern "C" int mft_dkt_backward(int episodes, int n_way, int n_support, int n_query, int D, int linear, const float* U,
                                const double* nrm, const float* A, const float* V, const float* B, const float* raw_outputscale,
                                const float* grad_loss, float* dfeats, int ldd, double* part, void* stream) {
    if (!dkt_shape_ok(episodes, n_way, n_support, n_query, D, 0) || U == nullptr || nrm == nullptr || A == nullptr || V == nullptr ||
        B == nullptr || raw_outputscale == nullptr || dfeats == nullptr || ldd < D || part == nullptr)
        return MFT_EINVAL;
    const int M = n_way * (n_support + n_query);
    hipLaunchKernelGGL(dkt_grad_kernel, dim3(cdiv(M, 4), episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, U, nrm, M, n_way, episodes,
                       linear ? 1 : 0, A, V, B, raw_outputscale, grad_loss, dfeats, ldd, part);
    return mft_launch_status();
}

extern "C" int mft_dkt_hyper_backward(int episodes, int n_way, int n_support, int n_query, int D, const double* part,
                                      const double* trace, const double* stats, const float* raw_outputscale, const float* raw_noise,
                                      const float* grad_loss, float* dmean, float* draw_outputscale, float* draw_noise, void* stream) {
    if (!dkt_shape_ok(episodes, n_way, n_support, n_query, D, 0) || part == nullptr || trace == nullptr || stats == nullptr ||
        raw_outputscale == nullptr ||
        raw_noise == nullptr || dmean == nullptr || draw_outputscale == nullptr || draw_noise == nullptr)
        return MFT_EINVAL;
    hipLaunchKernelGGL(dkt_hyper_kernel, dim3(1), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, part, trace, stats,
                       n_way * (n_support + n_query), n_way, episodes, raw_outputscale, raw_noise, grad_loss, dmean,
                       draw_outputscale, draw_noise);
    return mft_launch_status();
}

extern "C" int mft_dkt_scores(int episodes, int n_way, int n_support, int n_query, int D, const float* U, const float* W,
                              const float* mean, float* scores, void* stream) {
    if (!dkt_shape_ok(episodes, n_way, n_support, n_query, D, 1) || !dkt_rows_ok(U, D) || !dkt_rows_ok(W, D) || mean == nullptr ||
        scores == nullptr)
        return MFT_EINVAL;
    const RidgeShape s = dkt_points(n_way, n_support, n_query, 1);
    hipLaunchKernelGGL(dkt_scores_kernel, dim3(cdiv((long long)n_way * n_query, 16), episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream,
                       U, s, W, mean, scores);
    return mft_launch_status();
}
