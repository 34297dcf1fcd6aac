// MetaOptNet multi-class SVM head: the Crammer-Singer dual of every episode of a step, and its adjoint.
//
//   M = Z_S Z_S^T + I     alpha = argmin 1/2 tr(alpha^T M alpha) - tr(Y^T alpha)   s.t. alpha <= C Y, alpha 1 = 0     C = 0.1
//   W = Z_S^T alpha       scores = scale * Z_Q W   (mft_ridge_scores / mft_ridge_backward_query of csrc/ridge.hip)
//
// Layout and domain are those of csrc/ridge.hip.  M [episodes, S, S] is a float64 workspace (both triangles): in fp32 its rounding
// moves alpha by more than the smallest slack at the optimum.  One workgroup per episode solves in double: rounds of
// SVM_PG_STEPS accelerated projected-gradient steps (step 1 / max_i sum_j |M_ij| <= 1 / lambda_max, per-row projection onto the
// simplex {beta >= 0, beta 1 = C} of beta = C Y - alpha, momentum dropped when it points uphill), then conjugate gradients on the
// face of the current free set F = {alpha < C Y} (the face's subspace: zero off F, every row sums to zero), the largest feasible
// step along the face solution, and -- after a full step -- the sign test of the multipliers of the bound entries.  The backward
// (U = 0 off F, U 1 = 0, (M U + w 1^T)_F = A_F) is the same face solve with the forward's saved mask and right-hand side Z_S dW.
//
// Thread (i = tid % 256, q = tid / 256) owns row i of classes 8q .. 8q + 7 of every iterate in registers.  A product M P reads
// P from LDS (class-major, [class][256 rows]) and streams column i of M from L2 (lanes read consecutive addresses); row-wise
// operations (projection, row means) stage the operand in a second LDS plane and every thread of a row repeats them in the same
// order.  Workgroup-wide sums add per-wave butterfly sums in wave order: no atomics, bit-identical reruns.  No kernel waits for
// another workgroup.  Every loop is bounded by a shape argument or by MFT_SVM_MAX_PRODUCTS (products M x [S, n_way] per episode):
// reaching it stores status = 1 with the last iterate.  A non-finite M stores NaN in alpha and W and status = 1 at once.  The
// conjugate-gradient stop is relative: |r|^2 <= (1e-13)^2 |b_F|^2.
#include "ridge_common.h"

namespace {

constexpr int SVM_WG = RIDGE_WG;
constexpr int SVM_ROWS = RIDGE_MAX_S;       // rows of a plane: thread row = tid % 256
constexpr int SVM_CPT = 8;                  // classes per thread
constexpr int SVM_PG_STEPS = 50;
constexpr double SVM_C = 0.1;
constexpr double SVM_CG_RTOL = 1e-13;
static_assert(SVM_WG == SVM_ROWS * (RIDGE_MAX_WAY / SVM_CPT), "one thread per (row, eight classes)");

// ---------------------------------------------------------------------------------------------------------------- Gram
// M = Z_S Z_S^T + I in double, both triangles, in 32x32 tiles (the tile loop of ridge_gram_kernel)
__global__ __launch_bounds__(RIDGE_THREADS) void svm_gram_kernel(const float* __restrict__ feats, RidgeShape s, int tiles,
                                                                 double* __restrict__ M) {
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
    double* Me = M + (long long)e * S * S;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = ti * 32 + ty + 16 * u, j = tj * 32 + tx + 16 * v;
            if (i < S && j <= i) {
                Me[(long long)i * S + j] = acc[u][v] + (i == j ? 1.0 : 0.0);
                if (j < i) Me[(long long)j * S + i] = acc[u][v];
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------- workgroup
struct SvmCtx {
    const double* M;        // the episode's [S][S]
    double *sp, *sv, *sred; // LDS: product operand plane, row-operation plane (both [classes][256]), one slot per wave
    int S, n_way, i, c0;
    int mine;               // the thread's entry k of a plane is plane[mine + k * SVM_ROWS]
    bool row, act;          // i < S; c0 < n_way (uniform over the wave)
};

__device__ __forceinline__ double block_sum(double v, double* sred) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sred[0];
#pragma unroll
    for (int w = 1; w < SVM_WG / 64; ++w) t += sred[w];
    __syncthreads();
    return t;
}

// min over the workgroup (MIN) or max; a NaN operand is ignored, as by fmin / fmax
template <bool MIN>
__device__ __forceinline__ double block_extreme(double v, double* sred) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = MIN ? fmin(v, o) : fmax(v, o);
    }
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sred[0];
#pragma unroll
    for (int w = 1; w < SVM_WG / 64; ++w) t = MIN ? fmin(t, sred[w]) : fmax(t, sred[w]);
    __syncthreads();
    return t;
}

// the thread's eight entries into an LDS plane (entries outside the shape hold zero)
__device__ __forceinline__ void stage(const SvmCtx& x, double* plane, const double (&v)[SVM_CPT]) {
    if (!x.act) return;
    double* p = plane + x.mine;
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k) p[k * SVM_ROWS] = v[k];
}

__device__ __forceinline__ void unstage(const SvmCtx& x, const double* plane, double (&v)[SVM_CPT]) {
    const double* p = plane + x.mine;
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k) v[k] = x.act ? p[k * SVM_ROWS] : 0.0;
}

// acc = rows of M x (the plane sp) for the thread's entries; sp must be staged and the workgroup synchronised
__device__ __forceinline__ void product(const SvmCtx& x, double (&acc)[SVM_CPT]) {
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k) acc[k] = 0.0;
    if (!x.act) return;
    const double* col = x.M + (x.row ? x.i : 0);
    const double* p = x.sp + x.c0 * SVM_ROWS;
#pragma unroll 1
    for (int j = 0; j < x.S; ++j) {
        const double m = col[(long long)j * x.S];
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) acc[k] += m * p[k * SVM_ROWS + j];
    }
    if (!x.row) {
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) acc[k] = 0.0;
    }
}

// the mean over the row's free set of v (entries off the free set are zeroed in v)
__device__ __forceinline__ double face_row_mean(const SvmCtx& x, unsigned own, int cnt, double (&v)[SVM_CPT]) {
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k)
        if (!((own >> k) & 1)) v[k] = 0.0;
    stage(x, x.sv, v);
    __syncthreads();
    double sum = 0.0;
    for (int c = 0; c < x.n_way; ++c) sum += x.sv[c * SVM_ROWS + x.i];
    __syncthreads();
    return sum / (double)cnt;
}

// v -> its projection on the face's subspace: zero off the free set, minus the row's mean over the free set on it
__device__ __forceinline__ void face_project(const SvmCtx& x, unsigned own, int cnt, double (&v)[SVM_CPT]) {
    const double mean = face_row_mean(x, own, cnt, v);
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k)
        if ((own >> k) & 1) v[k] -= mean;
}

__device__ __forceinline__ double dot8(const double (&a)[SVM_CPT], const double (&b)[SVM_CPT]) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k) t += a[k] * b[k];
    return t;
}

// conjugate gradients for P M P sol = P b on the face (own: the thread's free bits, cnt: the row's free count); b is consumed.
// Returns the number of products.
__device__ __forceinline__ int face_cg(const SvmCtx& x, unsigned own, int cnt, double (&b)[SVM_CPT], double (&sol)[SVM_CPT],
                                       int max_it) {
    double q[SVM_CPT], p[SVM_CPT];
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k) {
        if (!((own >> k) & 1)) b[k] = 0.0;
        sol[k] = 0.0;
    }
    const double bb = block_sum(dot8(b, b), x.sred);
    face_project(x, own, cnt, b);                                // b is the residual r from here on
    stage(x, x.sp, b);
    double rr = block_sum(dot8(b, b), x.sred);
    int it = 0;
    while (it < max_it && rr > SVM_CG_RTOL * SVM_CG_RTOL * bb) {
        __syncthreads();
        product(x, q);
        face_project(x, own, cnt, q);
        unstage(x, x.sp, p);
        const double pq = block_sum(dot8(p, q), x.sred);
        ++it;
        if (!(pq > 0.0)) break;
        const double a = rr / pq;
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) {
            sol[k] += a * p[k];
            b[k] -= a * q[k];
        }
        const double rn = block_sum(dot8(b, b), x.sred);
        const double beta = rn / rr;
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) p[k] = b[k] + beta * p[k];
        stage(x, x.sp, p);
        rr = rn;
    }
    __syncthreads();
    return it;
}

// the row's projection onto {beta >= 0, beta 1 = C} of the staged row sv[.][i]: returns tau and the kept set (Michelot: entries
// at or below the kept set's mean excess leave; at most n_way passes)
__device__ __forceinline__ double simplex_threshold(const SvmCtx& x, unsigned& keep) {
    keep = x.n_way == 32 ? ~0u : (1u << x.n_way) - 1u;
    double tau = 0.0;
    for (int pass = 0; pass < x.n_way; ++pass) {
        double sum = 0.0;
        for (int c = 0; c < x.n_way; ++c)
            if ((keep >> c) & 1) sum += x.sv[c * SVM_ROWS + x.i];
        tau = (sum - SVM_C) / (double)__popc(keep);
        unsigned next = 0;
        for (int c = 0; c < x.n_way; ++c)
            if (((keep >> c) & 1) && x.sv[c * SVM_ROWS + x.i] > tau) next |= 1u << c;
        if (next == keep) break;
        keep = next;
    }
    return tau;
}

// the row's free set of the staged iterate beta: bit c = [sv[c][i] > 0]
__device__ __forceinline__ unsigned row_free_mask(const SvmCtx& x) {
    unsigned m = 0;
    if (x.row)
        for (int c = 0; c < x.n_way; ++c)
            if (x.sv[c * SVM_ROWS + x.i] > 0.0) m |= 1u << c;
    return m;
}

__device__ __forceinline__ SvmCtx svm_ctx(const double* M, int e, int S, int n_way, double* sdyn, double* sred) {
    SvmCtx x;
    const int planes = ((n_way + SVM_CPT - 1) / SVM_CPT) * SVM_CPT * SVM_ROWS;
    x.M = M + (long long)e * S * S;
    x.sp = sdyn;
    x.sv = sdyn + planes;
    x.sred = sred;
    x.S = S;
    x.n_way = n_way;
    x.i = threadIdx.x & (SVM_ROWS - 1);
    x.c0 = (threadIdx.x / SVM_ROWS) * SVM_CPT;
    x.mine = x.c0 * SVM_ROWS + x.i;
    x.row = x.i < S;
    x.act = x.c0 < n_way;
    for (int idx = threadIdx.x; idx < 2 * planes; idx += SVM_WG) sdyn[idx] = 0.0;
    __syncthreads();
    return x;
}

// ---------------------------------------------------------------------------------------------------------------- solve
// The iterate is beta = C Y - alpha (beta >= 0, beta 1 = C, free = beta > 0): f = 1/2 tr(beta^T M beta) - tr(H^T beta) with
// H = C M Y - Y, so that no entry needs its own bound.  work [episodes][1024 threads][2][8] holds each thread's entries of H and,
// during a face solve, of beta; a thread reads back only what it wrote.  On exit work[episode][0] holds the product count.
__global__ __launch_bounds__(SVM_WG) void svm_solve_kernel(const float* __restrict__ feats, RidgeShape s, const double* __restrict__ M,
                                                           int max_products, double* work, float* __restrict__ alpha,
                                                           unsigned char* __restrict__ free_out, float* __restrict__ W,
                                                           int* __restrict__ status) {
    extern __shared__ double sdyn[];
    __shared__ double sred[SVM_WG / 64];
    const int e = blockIdx.x, tid = threadIdx.x, S = s.n_way * s.ns;
    const float* ep = feats + (long long)e * s.n_way * (s.ns + s.nq) * s.ld;
    const SvmCtx x = svm_ctx(M, e, S, s.n_way, sdyn, sred);
    const int cls = x.i / s.ns;
    double* hk = work + ((long long)e * SVM_WG + tid) * (2 * SVM_CPT);
    double* park = hk + SVM_CPT;
    // step bound (Gershgorin) and the finite test: a NaN or an infinity anywhere in M reaches the sum
    double rs = 0.0;
    if (x.row && tid < SVM_ROWS)
        for (int j = 0; j < S; ++j) rs += fabs(x.M[(long long)j * S + x.i]);
    const double lip = block_extreme<false>(rs, sred), total = block_sum(rs, sred);
    const bool finite = total - total == 0.0;
    // H, and the start beta = C Y (alpha = 0)
    double b[SVM_CPT];
    unsigned valid = 0;
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k) {
        const int c = x.c0 + k;
        double h = 0.0;
        b[k] = 0.0;
        if (x.row && c < s.n_way) {
            valid |= 1u << k;
            for (int j = c * s.ns; j < (c + 1) * s.ns; ++j) h += x.M[(long long)j * S + x.i];
            h = SVM_C * h - (c == cls ? 1.0 : 0.0);
            if (c == cls) b[k] = SVM_C;
        }
        hk[k] = h;
    }
    int products = 0, st = 1;
    while (finite && products < max_products) {
        {   // accelerated projected gradient
            double bp[SVM_CPT], g[SVM_CPT];
#pragma unroll
            for (int k = 0; k < SVM_CPT; ++k) bp[k] = b[k];
            double t = 1.0;
            for (int step = 0; step < SVM_PG_STEPS; ++step) {
                double tn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t));
                const double mom = (t - 1.0) / tn;
#pragma unroll
                for (int k = 0; k < SVM_CPT; ++k) g[k] = b[k] + mom * (b[k] - bp[k]);
                stage(x, x.sp, g);
                __syncthreads();
                product(x, g);
#pragma unroll
                for (int k = 0; k < SVM_CPT; ++k) {
                    const double y = x.act ? x.sp[x.mine + k * SVM_ROWS] : 0.0;       // read back, not kept across the product
                    g[k] = y - (g[k] - hk[k]) / lip;
                }
                stage(x, x.sv, g);
                __syncthreads();
                unsigned keep;
                const double tau = simplex_threshold(x, keep);
                keep = x.row ? keep >> x.c0 : 0u;
                double up = 0.0;
#pragma unroll
                for (int k = 0; k < SVM_CPT; ++k) {
                    const double bn = (keep >> k) & 1 ? g[k] - tau : 0.0;
                    const double y = x.act ? x.sp[x.mine + k * SVM_ROWS] : 0.0;
                    up += (y - bn) * (bn - b[k]);
                    bp[k] = b[k];
                    b[k] = bn;
                }
                if (block_sum(up, sred) > 0.0) tn = 1.0;
                t = tn;
            }
            products += SVM_PG_STEPS;
        }
        double g[SVM_CPT], d[SVM_CPT];
        // the face of the iterate and minus the gradient on it
        stage(x, x.sv, b);
        stage(x, x.sp, b);
        __syncthreads();
        unsigned rowmask = row_free_mask(x);
        unsigned own = (rowmask >> x.c0) & 0xffu;
        product(x, g);
        ++products;
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) {
            g[k] = hk[k] - g[k];
            park[k] = b[k];                           // beta waits in the workspace: the face solve needs the registers
        }
        __syncthreads();
        products += face_cg(x, own, max(__popc(rowmask), 1), g, d, max_products - products);
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) b[k] = park[k];
        double ratio = __builtin_inf();
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k)
            if (d[k] < 0.0) ratio = fmin(ratio, b[k] / -d[k]);   // d is zero off the free set
        ratio = block_extreme<true>(ratio, sred);
        const double len = ratio < 1.0 ? ratio : 1.0;
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) {
            double bn = b[k] + len * d[k];
            if (len < 1.0 && d[k] < 0.0 && b[k] / -d[k] <= len) bn = 0.0;
            b[k] = fmax(bn, 0.0);
        }
        if (len < 1.0) continue;                                 // the step met a bound: the face has changed
        // a full step: the multipliers of the bound entries decide
        stage(x, x.sv, b);
        stage(x, x.sp, b);
        __syncthreads();
        rowmask = row_free_mask(x);
        own = (rowmask >> x.c0) & 0xffu;
        product(x, g);
        ++products;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k) {
            g[k] -= hk[k];
            d[k] = g[k];
        }
        const double w = -face_row_mean(x, own, max(__popc(rowmask), 1), d);     // g + w = 0 on the free set, mu = g + w off it
        const unsigned pass = own | ~valid;
        double bad = 0.0;
#pragma unroll
        for (int k = 0; k < SVM_CPT; ++k)
            if (!((pass >> k) & 1) && !(g[k] + w >= 0.0)) bad = 1.0;
        if (block_sum(bad, sred) == 0.0) {
            st = 0;
            break;
        }
    }
    // alpha = C Y - beta in fp32, never above its bound; the free mask of the double iterate; W = Z_S^T alpha from the stored alpha
    __syncthreads();
    float* coef = (float*)sdyn;
    float* ae = alpha + (long long)e * S * s.n_way;
    unsigned char* fe = free_out + (long long)e * S * s.n_way;
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k) {
        if (!((valid >> k) & 1)) continue;
        const double cy = x.c0 + k == cls ? SVM_C : 0.0;
        float af = (float)(cy - b[k]);
        if ((double)af > cy) af = nextafterf(af, -__builtin_inff());
        if (!finite) af = __builtin_nanf("");
        const int o = x.i * s.n_way + x.c0 + k;
        ae[o] = coef[o] = af;
        fe[o] = b[k] > 0.0 ? 1 : 0;
    }
    if (tid == 0) {
        status[e] = st;
        hk[0] = (double)products;                                // H is dead: the episode's product count, for the timing tool
    }
    __syncthreads();
    const int dcol = tid & (RIDGE_D - 1), c0 = (tid >> 9) * 16;
    double wv[16];
    support_combine(ep, s, S, dcol, c0, coef, wv);
    float* We = W + (long long)e * s.n_way * RIDGE_D;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc)
        if (c0 + cc < s.n_way) We[(c0 + cc) * RIDGE_D + dcol] = (float)wv[cc];
}

// ---------------------------------------------------------------------------------------------------------------- backward
// support side, one workgroup per episode: A = Z_S dW, the face solve for U on the saved mask, then the assembly of
// ridge_bwd_support_kernel with U in the place of B; workgroup 0 also sums the dscale shares in order
__global__ __launch_bounds__(SVM_WG) void svm_bwd_support_kernel(const float* __restrict__ feats, RidgeShape s, int episodes,
                                                                 const double* __restrict__ M, int max_products,
                                                                 const float* __restrict__ alpha,
                                                                 const unsigned char* __restrict__ free_in,
                                                                 const float* __restrict__ W, const float* __restrict__ dW,
                                                                 const double* __restrict__ dscale_part, float* __restrict__ dfeats,
                                                                 int ldd, float* __restrict__ dscale) {
    extern __shared__ double sdyn[];
    __shared__ double sred[SVM_WG / 64];
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
    const SvmCtx x = svm_ctx(M, e, S, s.n_way, sdyn, sred);
    // A [n_way][256] into the row plane, one wave per support row
    for (int i = wave; i < S; i += SVM_WG / 64) {
        const float* z = sup_row(ep, s, i);
        const f32x4 z0 = *(const f32x4*)(z + 4 * lane), z1 = *(const f32x4*)(z + 256 + 4 * lane);
        for (int c = 0; c < s.n_way; ++c) {
            const f32x4* wr = (const f32x4*)(dWe + c * RIDGE_D);
            const double p = group_sum<64>(dot4(z0, wr[lane]) + dot4(z1, wr[64 + lane]));
            if (lane == 0) x.sv[c * SVM_ROWS + i] = p;
        }
    }
    __syncthreads();
    const unsigned char* fe = free_in + (long long)e * S * s.n_way;
    unsigned rowmask = 0;
    if (x.row)
        for (int c = 0; c < s.n_way; ++c)
            if (fe[x.i * s.n_way + c]) rowmask |= 1u << c;
    const unsigned own = (rowmask >> x.c0) & 0xffu;
    double b[SVM_CPT], u[SVM_CPT];
    unstage(x, x.sv, b);                                         // rows and classes outside the shape hold zero
    __syncthreads();
    face_cg(x, own, max(__popc(rowmask), 1), b, u, max_products);
    // the planes are dead: alpha, U [S][n_way] and dW - Z_S^T U [n_way][D] follow
    float* sa = (float*)sdyn;
    float* sb = sa + S * s.n_way;
    float* sm = sa + 2 * S * s.n_way;
    const float* ae = alpha + (long long)e * S * s.n_way;
    for (int i = tid; i < S * s.n_way; i += SVM_WG) sa[i] = ae[i];
#pragma unroll
    for (int k = 0; k < SVM_CPT; ++k)
        if (x.row && x.c0 + k < s.n_way) sb[x.i * s.n_way + x.c0 + k] = (float)u[k];
    __syncthreads();
    support_assemble(ep, s, S, tid, sa, sb, sm, We, dWe, dep, ldd);
}

// both planes for n_way rounded up to the classes of a thread: 131,072 bytes at n_way = 32; the backward's assembly
// (2 S n_way + n_way D floats) fits in them for every S <= 256
size_t svm_lds(int n_way) { return (size_t)2 * ((n_way + SVM_CPT - 1) / SVM_CPT) * SVM_CPT * SVM_ROWS * sizeof(double); }

constexpr int SVM_MAX_LDS = 2 * RIDGE_MAX_WAY * SVM_ROWS * 8;
static_assert(SVM_MAX_LDS + 1024 <= 160 * 1024, "one CU's LDS");
static_assert(4 * (2 * RIDGE_MAX_S + RIDGE_D) <= 2 * SVM_ROWS * 8, "the assembly fits per class");

template <typename K>
int svm_lds_attr(K kern, MftPerDeviceOnce& once) {
    if (once.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SVM_MAX_LDS);
        if (e != hipSuccess) return (int)e;
        once.mark();
    }
    return 0;
}

}  // namespace

extern "C" int mft_svm_gram(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, double* M,
                            void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || M == nullptr) return MFT_EINVAL;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    const int tiles = cdiv(n_way * n_support, 32);
    hipLaunchKernelGGL(svm_gram_kernel, dim3(tiles * tiles, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, feats, s, tiles, M);
    return mft_launch_status();
}

extern "C" int mft_svm_solve(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, const double* M,
                             double* work, float* alpha, unsigned char* free_mask, float* W, int* status, void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || M == nullptr || work == nullptr ||
        alpha == nullptr || free_mask == nullptr || W == nullptr || status == nullptr)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = svm_lds_attr(svm_solve_kernel, once);
    if (rc != 0) return rc;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(svm_solve_kernel, dim3(episodes), dim3(SVM_WG), svm_lds(n_way), (hipStream_t)stream, feats, s, M,
                       MFT_SVM_MAX_PRODUCTS, work, alpha, free_mask, W, status);
    return mft_launch_status();
}

extern "C" int mft_svm_backward_support(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                        const double* M, const float* alpha, const unsigned char* free_mask, const float* W,
                                        const float* dW, const double* dscale_part, float* dfeats, int ldd, float* dscale,
                                        void* stream) {
    if (!ridge_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || M == nullptr || alpha == nullptr ||
        free_mask == nullptr || W == nullptr || dW == nullptr || dscale_part == nullptr || dfeats == nullptr || dscale == nullptr)
        return MFT_EINVAL;
    if (ldd < D || ((uintptr_t)dW & 15) != 0) return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = svm_lds_attr(svm_bwd_support_kernel, once);
    if (rc != 0) return rc;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    hipLaunchKernelGGL(svm_bwd_support_kernel, dim3(episodes), dim3(SVM_WG), svm_lds(n_way), (hipStream_t)stream, feats, s, episodes,
                       M, MFT_SVM_MAX_PRODUCTS, alpha, free_mask, W, dW, dscale_part, dfeats, ldd, dscale);
    return mft_launch_status();
}
