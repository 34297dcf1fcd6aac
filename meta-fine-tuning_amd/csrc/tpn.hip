// Transductive Propagation Network head forward and backward, every episode of a step per launch.
//
//   sigma = fc4(relu(fc3 z))   u = z / (sigma + EPS)   W_ij = exp(-|u_i - u_j|^2 / 2)   W <- W * mask (k largest per row, OR transpose)
//   D_j = sum_i W_ij   S = D^-1/2 W D^-1/2   F = (I - alpha S)^-1 Y   scores = the query rows of F
//
// Layout: feats as for csrc/ridge.hip ([episodes, n_way, n_support + n_query, D = 512], row stride ld).  NODE n of an episode is
// support row n (class-major) for n < S = n_way * n_support and query row n - S (class-major) after that; N = n_way * (n_support +
// n_query) <= 256 nodes.  u [episodes, N, D], W / mask / dd [episodes, N, N], F [episodes, N, n_way], rinv [episodes, N] and the
// packed factor L [episodes, N (N + 1) / 2] are in node order; hid [rows, 8], sig [rows] (float64) and dnode [rows, 9] (float64) are
// in the row order of feats.
//
// Storage is fp32; every sum, the exponential, both triangular solves and the normalisation run in double inside the kernels and
// round once on the store.  No atomics; every sum runs in a fixed order, so two launches on the same input are bit-identical and
// an episode's result does not depend on the episodes beside it.  No kernel waits for another workgroup, and the trip count of
// every loop is a function of the shape arguments alone (the neighbour selection counts ranks, it does not sort): a non-finite
// feature gives non-finite output and the launch returns.
#include "ridge_common.h"

namespace {

constexpr int TPN_MAX_N = 256;
constexpr int TPN_HID = 8;
constexpr int TPN_DN = TPN_HID + 1;                 // dnode row: d(loss)/d(hidden pre-activation) x 8, d(loss)/d(sigma)
static_assert(RIDGE_THREADS / 64 == 4, "tpn_param_bwd_kernel adds four partial sums");
constexpr double TPN_EPS = 2.220446049250313e-16;   // np.finfo(float).eps

// feats row (within the episode) of node n
__device__ __forceinline__ int node_row(const RidgeShape s, int n) {
    const int S = s.n_way * s.ns;
    if (n < S) {
        const int c = n / s.ns;
        return c * (s.ns + s.nq) + (n - c * s.ns);
    }
    return (int)qry_row(s, n - S);
}

// node of feats row r (within the episode)
__device__ __forceinline__ int row_node(const RidgeShape s, int r) {
    const int c = r / (s.ns + s.nq), p = r - c * (s.ns + s.nq);
    return p < s.ns ? c * s.ns + p : s.n_way * s.ns + c * s.nq + (p - s.ns);
}

// ---------------------------------------------------------------------------------------------------------------- embed
// one wave per feats row: the 8 hidden pre-activations, s = sigma + EPS, u = z / s (written at the row's node)
__global__ __launch_bounds__(RIDGE_THREADS) void tpn_embed_kernel(const float* __restrict__ feats, RidgeShape s, int rows,
                                                                  const float* __restrict__ w3, const float* __restrict__ b3,
                                                                  const float* __restrict__ w4, const float* __restrict__ b4,
                                                                  float* __restrict__ u, float* __restrict__ hid,
                                                                  double* __restrict__ sig) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * (RIDGE_THREADS / 64) + wave;
    if (g >= rows) return;                                       // uniform over the wave
    const int N = s.n_way * (s.ns + s.nq);
    const int e = g / N, r = g - e * N;
    const float* x = feats + (long long)g * s.ld;
    const f32x4 x0 = *(const f32x4*)(x + 4 * lane), x1 = *(const f32x4*)(x + 256 + 4 * lane);
    double sigma = (double)b4[0];
#pragma unroll
    for (int m = 0; m < TPN_HID; ++m) {
        const f32x4* wr = (const f32x4*)(w3 + m * RIDGE_D);
        const float h = (float)(group_sum<64>(dot4(x0, wr[lane]) + dot4(x1, wr[64 + lane])) + (double)b3[m]);
        if (lane == m) hid[(long long)g * TPN_HID + m] = h;
        sigma += (double)w4[m] * (h > 0.f ? (double)h : 0.0);
    }
    const double sv = sigma + TPN_EPS;
    if (lane == 0) sig[g] = sv;
    float* ur = u + ((long long)e * N + row_node(s, r)) * RIDGE_D;
    f32x4 o0, o1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o0[q] = (float)((double)x0[q] / sv);
        o1[q] = (float)((double)x1[q] / sv);
    }
    *(f32x4*)(ur + 4 * lane) = o0;
    *(f32x4*)(ur + 256 + 4 * lane) = o1;
}

// ---------------------------------------------------------------------------------------------------------------- affinity
// W = exp(-|u_i - u_j|^2 / 2) from direct differences, 32x32 tiles of the lower triangle, one tile per workgroup, 2x2 entries per
// thread; an off-diagonal tile also writes its transpose, so W is symmetric bit for bit
__global__ __launch_bounds__(RIDGE_THREADS) void tpn_affinity_kernel(const float* __restrict__ u, int N, int tiles,
                                                                     float* __restrict__ W) {
    __shared__ float sa[32][33], sb[32][33];
    const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles;
    if (tj > ti) return;
    const int e = blockIdx.y;
    const float* ue = u + (long long)e * N * RIDGE_D;
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int ia = ti * 32 + lr, ib = tj * 32 + lr;
    const float* pa = ia < N ? ue + (long long)ia * RIDGE_D : nullptr;
    const float* pb = ib < N ? ue + (long long)ib * RIDGE_D : nullptr;
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
            const double d00 = a0 - b0, d01 = a0 - b1, d10 = a1 - b0, d11 = a1 - b1;
            acc[0][0] += d00 * d00;
            acc[0][1] += d01 * d01;
            acc[1][0] += d10 * d10;
            acc[1][1] += d11 * d11;
        }
    }
    float* We = W + (long long)e * N * N;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i = ti * 32 + ty + 16 * a, j = tj * 32 + tx + 16 * b;
            if (i < N && j < N) {
                const float w = (float)exp(-0.5 * acc[a][b]);
                We[(long long)i * N + j] = w;
                if (ti != tj) We[(long long)j * N + i] = w;
            }
        }
}

__device__ __forceinline__ bool sel_bit(const unsigned int* __restrict__ bits, int i, int j) {
    return (bits[i * (TPN_MAX_N / 32) + (j >> 5)] >> (j & 31)) & 1u;
}

// ---------------------------------------------------------------------------------------------------------------- propagate
// one workgroup per episode: neighbour selection by rank count (or mask_in) into a bit mask in LDS, its symmetrisation, degrees,
// I - alpha S into the packed lower triangle in LDS, left-looking Cholesky (four threads per row), F = (I - alpha S)^-1 Y
__global__ __launch_bounds__(RIDGE_WG) void tpn_propagate_kernel(const float* __restrict__ W, RidgeShape s, int k, float alpha,
                                                                 const unsigned char* __restrict__ mask_in, float* __restrict__ L,
                                                                 float* __restrict__ F, unsigned char* __restrict__ mask,
                                                                 float* __restrict__ rinv, float* __restrict__ scores) {
    extern __shared__ float sl[];                                // selection: one staged row per wave; then the packed triangle
    __shared__ unsigned int sbits[TPN_MAX_N * (TPN_MAX_N / 32)];
    __shared__ float sr[TPN_MAX_N];
    __shared__ double sdiag;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = s.n_way * s.ns, N = s.n_way * (s.ns + s.nq);
    const float* We = W + (long long)e * N * N;
    const unsigned char* min_e = mask_in ? mask_in + (long long)e * N * N : nullptr;

    // entry j of row i is selected iff fewer than k entries of the row beat it under (value descending, index ascending)
    for (int i0 = 0; i0 < N; i0 += RIDGE_WG / 64) {
        const int i = i0 + wave;
        const bool live = i < N;
        float* srow = sl + wave * TPN_MAX_N;
        float mine[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = 64 * q + lane;
            mine[q] = (live && j < N) ? We[(long long)i * N + j] : 0.f;
            if (live && j < N) srow[j] = mine[q];
        }
        __syncthreads();
        if (live) {
            int cnt[4] = {0, 0, 0, 0};
            if (min_e == nullptr) {
                for (int jp = 0; jp < N; ++jp) {
                    const float v = srow[jp];
#pragma unroll
                    for (int q = 0; q < 4; ++q) cnt[q] += (v > mine[q] || (v == mine[q] && jp < 64 * q + lane)) ? 1 : 0;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 64 * q + lane;
                const bool keep = j < N && (min_e ? min_e[(long long)i * N + j] != 0 : cnt[q] < k);
                const unsigned long long b = __ballot(keep);
                if (lane == 0) {
                    sbits[i * (TPN_MAX_N / 32) + 2 * q] = (unsigned int)b;
                    sbits[i * (TPN_MAX_N / 32) + 2 * q + 1] = (unsigned int)(b >> 32);
                }
            }
        }
        __syncthreads();
    }

    // symmetrised mask out, degrees D_i = sum_j (W * mask)_ij (W is symmetric bit for bit), D^-1/2
    for (int i = wave; i < N; i += RIDGE_WG / 64) {
        double d = 0.0;
        for (int j = lane; j < N; j += 64) {
            const bool m = sel_bit(sbits, i, j) || sel_bit(sbits, j, i);
            if (mask) mask[(long long)e * N * N + (long long)i * N + j] = m ? 1 : 0;
            d += m ? (double)We[(long long)i * N + j] : 0.0;
        }
        d = group_sum<64>(d);
        if (lane == 0) {
            const float r = (float)sqrt(1.0 / (d + TPN_EPS));
            sr[i] = r;
            if (rinv) rinv[(long long)e * N + i] = r;
        }
    }
    __syncthreads();

    for (int idx = tid; idx < N * N; idx += RIDGE_WG) {
        const int i = idx / N, j = idx - i * N;
        if (j <= i) {
            const bool m = sel_bit(sbits, i, j) || sel_bit(sbits, j, i);
            const double w = m ? (double)We[idx] : 0.0;
            sl[i * (i + 1) / 2 + j] = (float)((i == j ? 1.0 : 0.0) - (double)alpha * (double)sr[i] * w * (double)sr[j]);
        }
    }
    __syncthreads();
    // 1024 threads over N rows: 4 threads per row up to 256 rows, 8 up to 128, 16 up to 64 (a function of the shape alone)
    if (N > 128) cholesky_packed<4>(sl, N, tid, &sdiag);
    else if (N > 64) cholesky_packed<8>(sl, N, tid, &sdiag);
    else cholesky_packed<16>(sl, N, tid, &sdiag);
    const int packed = N * (N + 1) / 2;
    if (L) {
        float* Le = L + (long long)e * packed;
        for (int idx = tid; idx < packed; idx += RIDGE_WG) Le[idx] = sl[idx];
    }
    const int c = tid >> 5, part = tid & 31;
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        v[t] = (j < S && j / s.ns == c) ? 1.0 : 0.0;
    }
    solve_lower(sl, N, part, v);
    solve_lower_transposed(sl, N, part, v);
    const int Q = s.n_way * s.nq;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        if (j < N && c < s.n_way) {
            const float f = (float)v[t];
            if (F) F[((long long)e * N + j) * s.n_way + c] = f;
            if (j >= S) scores[((long long)e * Q + (j - S)) * s.n_way + c] = f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// one workgroup per episode: Lambda = (I - alpha S)^-1 dF from the saved factor; with P = alpha (Lambda F^T + F Lambda^T),
// dr_i = sum_j P_ij (W mask)_ij r_j, dD_i = -r_i^3 dr_i / 2 and
//   dd_ij = -(W mask)_ij (r_i r_j P_ij + dD_i + dD_j) / 2
// is the gradient with respect to the squared distance of the pair {i, j}, both orders of the pair added (dd is symmetric)
__global__ __launch_bounds__(RIDGE_WG) void tpn_propagate_bwd_kernel(const float* __restrict__ W, RidgeShape s, float alpha,
                                                                     const float* __restrict__ L, const float* __restrict__ F,
                                                                     const unsigned char* __restrict__ mask,
                                                                     const float* __restrict__ rinv, const float* __restrict__ dscores,
                                                                     int ldg, float* __restrict__ dd) {
    extern __shared__ float sl[];
    __shared__ float sr[TPN_MAX_N];
    __shared__ double sdd[TPN_MAX_N];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = s.n_way * s.ns, N = s.n_way * (s.ns + s.nq), Q = s.n_way * s.nq, nw = s.n_way;
    const float* We = W + (long long)e * N * N;
    const unsigned char* me = mask + (long long)e * N * N;
    const int packed = N * (N + 1) / 2;
    const float* Le = L + (long long)e * packed;
    for (int idx = tid; idx < packed; idx += RIDGE_WG) sl[idx] = Le[idx];
    if (tid < N) sr[tid] = rinv[(long long)e * N + tid];
    const int c = tid >> 5, part = tid & 31;
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        v[t] = (j >= S && j < N && c < nw) ? (double)dscores[((long long)e * Q + (j - S)) * ldg + c] : 0.0;
    }
    __syncthreads();
    solve_lower(sl, N, part, v);
    solve_lower_transposed(sl, N, part, v);
    __syncthreads();                                             // L is dead: Lambda and F [N][n_way] follow
    float* slam = sl;
    float* sf = sl + N * nw;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = 32 * t + part;
        if (j < N && c < nw) slam[j * nw + c] = (float)v[t];
    }
    const float* Fe = F + (long long)e * N * nw;
    for (int idx = tid; idx < N * nw; idx += RIDGE_WG) sf[idx] = Fe[idx];
    __syncthreads();
    for (int i = wave; i < N; i += RIDGE_WG / 64) {
        double acc = 0.0;
        for (int j = lane; j < N; j += 64) {
            if (me[(long long)i * N + j]) {
                double p = 0.0;
                for (int cc = 0; cc < nw; ++cc)
                    p += (double)slam[i * nw + cc] * (double)sf[j * nw + cc] + (double)slam[j * nw + cc] * (double)sf[i * nw + cc];
                acc += (double)alpha * p * (double)We[(long long)i * N + j] * (double)sr[j];
            }
        }
        acc = group_sum<64>(acc);
        const double r = sr[i];
        if (lane == 0) sdd[i] = -0.5 * r * r * r * acc;
    }
    __syncthreads();
    float* dde = dd + (long long)e * N * N;
    for (int idx = tid; idx < N * N; idx += RIDGE_WG) {
        const int i = idx / N, j = idx - i * N;
        double t = 0.0;
        if (me[idx]) {
            double p = 0.0;
            for (int cc = 0; cc < nw; ++cc)
                p += (double)slam[i * nw + cc] * (double)sf[j * nw + cc] + (double)slam[j * nw + cc] * (double)sf[i * nw + cc];
            t = -0.5 * (double)We[idx] * ((double)sr[i] * (double)sr[j] * (double)alpha * p + sdd[i] + sdd[j]);
        }
        dde[idx] = (float)t;
    }
}

// four nodes per workgroup, two columns per thread: du_i = 2 sum_j dd_ij (u_i - u_j) from direct differences, then through
// u = z / s and the two linear layers: dz = du / s + sum_m dh_m fc3_m, dsigma = -(du . u) / s, dh_m = dsigma fc4_m [h_m > 0]
__global__ __launch_bounds__(RIDGE_THREADS) void tpn_affinity_bwd_kernel(RidgeShape s, const float* __restrict__ u,
                                                                         const float* __restrict__ hid, const double* __restrict__ sig,
                                                                         const float* __restrict__ dd, const float* __restrict__ w3,
                                                                         const float* __restrict__ w4, float* __restrict__ dfeats,
                                                                         int ldd, double* __restrict__ dnode) {
    __shared__ double sred[4][RIDGE_THREADS / 64];
    const int e = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = s.n_way * (s.ns + s.nq), i0 = blockIdx.x * 4;
    const float* ue = u + (long long)e * N * RIDGE_D;
    const float* dde = dd + (long long)e * N * N;
    const int d0 = tid, d1 = tid + RIDGE_THREADS;
    double ui[4][2], acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool live = i0 + q < N;
        ui[q][0] = live ? (double)ue[(long long)(i0 + q) * RIDGE_D + d0] : 0.0;
        ui[q][1] = live ? (double)ue[(long long)(i0 + q) * RIDGE_D + d1] : 0.0;
        acc[q][0] = acc[q][1] = 0.0;
    }
    for (int j = 0; j < N; ++j) {
        const double uj0 = ue[(long long)j * RIDGE_D + d0], uj1 = ue[(long long)j * RIDGE_D + d1];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double t = i0 + q < N ? (double)dde[(long long)(i0 + q) * N + j] : 0.0;
            acc[q][0] += t * (ui[q][0] - uj0);
            acc[q][1] += t * (ui[q][1] - uj1);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q][0] *= 2.0;
        acc[q][1] *= 2.0;
        const double p = group_sum<64>(acc[q][0] * ui[q][0] + acc[q][1] * ui[q][1]);
        if (lane == 0) sred[q][wave] = p;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (i0 + q >= N) continue;                               // uniform over the workgroup
        const long long g = (long long)e * N + node_row(s, i0 + q);
        const double sv = sig[g];
        const double dsig = -(((sred[q][0] + sred[q][1]) + sred[q][2]) + sred[q][3]) / sv;
        double z0 = acc[q][0] / sv, z1 = acc[q][1] / sv;
#pragma unroll
        for (int m = 0; m < TPN_HID; ++m) {
            const double dh = hid[g * TPN_HID + m] > 0.f ? dsig * (double)w4[m] : 0.0;
            z0 += dh * (double)w3[m * RIDGE_D + d0];
            z1 += dh * (double)w3[m * RIDGE_D + d1];
            if (tid == m) dnode[g * TPN_DN + m] = dh;
        }
        if (tid == TPN_HID) dnode[g * TPN_DN + TPN_HID] = dsig;
        dfeats[g * ldd + d0] = (float)z0;
        dfeats[g * ldd + d1] = (float)z1;
    }
}

// the four parameter gradients, each summed over the rows of feats in an order that depends on the row count alone: workgroups
// 0..7 the 8 x 64 columns of d(fc3.weight), workgroup 8 d(fc3.bias), d(fc4.weight) and d(fc4.bias)
__global__ __launch_bounds__(RIDGE_THREADS) void tpn_param_bwd_kernel(const float* __restrict__ feats, int ld, int rows,
                                                                      const float* __restrict__ hid, const double* __restrict__ dnode,
                                                                      float* __restrict__ dw3, float* __restrict__ db3,
                                                                      float* __restrict__ dw4, float* __restrict__ db4) {
    __shared__ double spart[RIDGE_THREADS / 64][TPN_HID][64];
    const int tid = threadIdx.x;
    if (blockIdx.x < RIDGE_CB) {
        // 64 columns per workgroup; wave w sums the w-th quarter of the rows, then the four quarters are added in order
        const int lane = tid & 63, wave = tid >> 6, d = blockIdx.x * 64 + lane;
        const int per = (rows + RIDGE_THREADS / 64 - 1) / (RIDGE_THREADS / 64);
        const int g1 = min(rows, (wave + 1) * per);
        double acc[TPN_HID];
#pragma unroll
        for (int m = 0; m < TPN_HID; ++m) acc[m] = 0.0;
        for (int g = wave * per; g < g1; ++g) {
            const double z = feats[(long long)g * ld + d];
#pragma unroll
            for (int m = 0; m < TPN_HID; ++m) acc[m] += dnode[(long long)g * TPN_DN + m] * z;
        }
#pragma unroll
        for (int m = 0; m < TPN_HID; ++m) spart[wave][m][lane] = acc[m];
        __syncthreads();
        for (int m = wave; m < TPN_HID; m += RIDGE_THREADS / 64)
            dw3[m * RIDGE_D + d] = (float)(((spart[0][m][lane] + spart[1][m][lane]) + spart[2][m][lane]) + spart[3][m][lane]);
        return;
    }
    // the 17 small sums, one per wave in turn: the lanes stride over the rows, a butterfly adds the 64 partial sums
    const int lane = tid & 63, wave = tid >> 6;
    for (int item = wave; item <= 2 * TPN_HID; item += RIDGE_THREADS / 64) {
        const int m = item & (TPN_HID - 1);
        double acc = 0.0;
        for (int g = lane; g < rows; g += 64) {
            if (item < TPN_HID) {
                acc += dnode[(long long)g * TPN_DN + m];
            } else if (item < 2 * TPN_HID) {
                const float h = hid[(long long)g * TPN_HID + m];
                acc += dnode[(long long)g * TPN_DN + TPN_HID] * (h > 0.f ? (double)h : 0.0);
            } else {
                acc += dnode[(long long)g * TPN_DN + TPN_HID];
            }
        }
        acc = group_sum<64>(acc);
        if (lane == 0) {
            if (item < TPN_HID) db3[m] = (float)acc;
            else if (item < 2 * TPN_HID) dw4[m] = (float)acc;
            else db4[0] = (float)acc;
        }
    }
}

inline bool tpn_shape_ok(int episodes, int n_way, int n_support, int n_query, int D) {
    if (episodes < 1 || n_way < 1 || n_way > RIDGE_MAX_WAY || n_support < 1 || n_query < 1 || D != RIDGE_D) return false;
    return (long long)n_way * ((long long)n_support + n_query) <= TPN_MAX_N;
}

inline bool tpn_rows_ok(const void* p, int ld) { return p != nullptr && ld >= RIDGE_D && (ld & 3) == 0 && ((uintptr_t)p & 15) == 0; }

// the largest dynamic LDS either one-workgroup kernel asks for: the packed triangle at N = 256 (131,584 bytes); beside it the
// forward keeps 9,224 bytes and the backward 3,072 bytes of static LDS
constexpr int TPN_MAX_LDS = 4 * (TPN_MAX_N * (TPN_MAX_N + 1) / 2);
static_assert(TPN_MAX_LDS + 4 * TPN_MAX_N * (TPN_MAX_N / 32) + 4 * TPN_MAX_N + 8 <= 160 * 1024, "forward: one CU's LDS");
static_assert(TPN_MAX_LDS + 4 * TPN_MAX_N + 8 * TPN_MAX_N <= 160 * 1024, "backward: one CU's LDS");
static_assert(4 * (RIDGE_WG / 64) * TPN_MAX_N <= TPN_MAX_LDS && 4 * 2 * TPN_MAX_N * RIDGE_MAX_WAY <= TPN_MAX_LDS, "the other uses fit");

size_t propagate_lds(int N) {
    const size_t packed = 4 * ((size_t)N * (N + 1) / 2), stage = 4 * (size_t)(RIDGE_WG / 64) * TPN_MAX_N;
    return packed > stage ? packed : stage;
}

size_t propagate_bwd_lds(int N, int n_way) {
    const size_t packed = 4 * ((size_t)N * (N + 1) / 2), tail = 4 * 2 * (size_t)N * n_way;
    return packed > tail ? packed : tail;
}

template <typename K>
int tpn_lds_attr(K kern, MftPerDeviceOnce& once) {
    if (once.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, TPN_MAX_LDS);
        if (e != hipSuccess) return (int)e;
        once.mark();
    }
    return 0;
}

}  // namespace

extern "C" int mft_tpn_embed(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, const float* w3,
                             const float* b3, const float* w4, const float* b4, float* u, float* hid, double* sig, void* stream) {
    if (!tpn_shape_ok(episodes, n_way, n_support, n_query, D) || !tpn_rows_ok(feats, ld) || !tpn_rows_ok(w3, D) || !tpn_rows_ok(u, D) ||
        b3 == nullptr || w4 == nullptr || b4 == nullptr || hid == nullptr || sig == nullptr)
        return MFT_EINVAL;
    const RidgeShape s = {n_way, n_support, n_query, ld};
    const int rows = episodes * n_way * (n_support + n_query);
    hipLaunchKernelGGL(tpn_embed_kernel, dim3(cdiv(rows, RIDGE_THREADS / 64)), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, feats, s, rows,
                       w3, b3, w4, b4, u, hid, sig);
    return mft_launch_status();
}

extern "C" int mft_tpn_affinity(int episodes, int n_way, int n_support, int n_query, int D, const float* u, float* W, void* stream) {
    if (!tpn_shape_ok(episodes, n_way, n_support, n_query, D) || !tpn_rows_ok(u, D) || W == nullptr) return MFT_EINVAL;
    const int N = n_way * (n_support + n_query), tiles = cdiv(N, 32);
    hipLaunchKernelGGL(tpn_affinity_kernel, dim3(tiles * tiles, episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, u, N, tiles, W);
    return mft_launch_status();
}

extern "C" int mft_tpn_propagate(int episodes, int n_way, int n_support, int n_query, int D, const float* W, int k, float alpha,
                                 const unsigned char* mask_in, float* L, float* F, unsigned char* mask, float* rinv, float* scores,
                                 void* stream) {
    if (!tpn_shape_ok(episodes, n_way, n_support, n_query, D) || k < 1 || k > TPN_MAX_N || W == nullptr || scores == nullptr)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = tpn_lds_attr(tpn_propagate_kernel, once);
    if (rc != 0) return rc;
    const RidgeShape s = {n_way, n_support, n_query, D};
    hipLaunchKernelGGL(tpn_propagate_kernel, dim3(episodes), dim3(RIDGE_WG), propagate_lds(n_way * (n_support + n_query)),
                       (hipStream_t)stream, W, s, k, alpha, mask_in, L, F, mask, rinv, scores);
    return mft_launch_status();
}

extern "C" int mft_tpn_propagate_backward(int episodes, int n_way, int n_support, int n_query, int D, const float* W, float alpha,
                                          const float* L, const float* F, const unsigned char* mask, const float* rinv,
                                          const float* dscores, int ldg, float* dd, void* stream) {
    if (!tpn_shape_ok(episodes, n_way, n_support, n_query, D) || W == nullptr || L == nullptr || F == nullptr || mask == nullptr ||
        rinv == nullptr || dscores == nullptr || dd == nullptr || ldg < n_way)
        return MFT_EINVAL;
    static MftPerDeviceOnce once;
    const int rc = tpn_lds_attr(tpn_propagate_bwd_kernel, once);
    if (rc != 0) return rc;
    const RidgeShape s = {n_way, n_support, n_query, D};
    hipLaunchKernelGGL(tpn_propagate_bwd_kernel, dim3(episodes), dim3(RIDGE_WG), propagate_bwd_lds(n_way * (n_support + n_query), n_way),
                       (hipStream_t)stream, W, s, alpha, L, F, mask, rinv, dscores, ldg, dd);
    return mft_launch_status();
}

extern "C" int mft_tpn_affinity_backward(int episodes, int n_way, int n_support, int n_query, int D, const float* u, const float* hid,
                                         const double* sig, const float* dd, const float* w3, const float* w4, float* dfeats, int ldd,
                                         double* dnode, void* stream) {
    if (!tpn_shape_ok(episodes, n_way, n_support, n_query, D) || u == nullptr || hid == nullptr || sig == nullptr || dd == nullptr ||
        w3 == nullptr || w4 == nullptr || dfeats == nullptr || dnode == nullptr || ldd < D)
        return MFT_EINVAL;
    const RidgeShape s = {n_way, n_support, n_query, D};
    const int N = n_way * (n_support + n_query);
    hipLaunchKernelGGL(tpn_affinity_bwd_kernel, dim3(cdiv(N, 4), episodes), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, s, u, hid, sig,
                       dd, w3, w4, dfeats, ldd, dnode);
    return mft_launch_status();
}

extern "C" int mft_tpn_param_backward(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                      const float* hid, const double* dnode, float* dw3, float* db3, float* dw4, float* db4,
                                      void* stream) {
    if (!tpn_shape_ok(episodes, n_way, n_support, n_query, D) || !tpn_rows_ok(feats, ld) || hid == nullptr || dnode == nullptr ||
        dw3 == nullptr || db3 == nullptr || dw4 == nullptr || db4 == nullptr)
        return MFT_EINVAL;
    const int rows = episodes * n_way * (n_support + n_query);
    hipLaunchKernelGGL(tpn_param_bwd_kernel, dim3(RIDGE_CB + 1), dim3(RIDGE_THREADS), 0, (hipStream_t)stream, feats, ld, rows, hid, dnode, dw3, db3,
                       dw4, db4);
    return mft_launch_status();
}
