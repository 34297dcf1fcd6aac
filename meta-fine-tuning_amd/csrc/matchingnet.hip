// MatchingNet head: bidirectional support LSTM (G_encoder), attention LSTM over the queries (FCE), cosine
// read-out and NLL loss, forward and backward, every episode of a lockstep step in one launch.
//
// The recurrence is cut at launch boundaries: one launch sequence per time step (the step is replayed from a hipGraph), no kernel
// waits for another workgroup.  Everything is fp32 with accurate expf / tanhf; every sum runs in a fixed order (no atomics), so
// two runs on the same input are bit-identical.  Weight gradients are NOT accumulated step by step: the backward steps leave
// d(gate pre-activations) of every time step in place of the saved gates and ONE transposed GEMM per weight sums over all steps.
//
// Layouts (D = 512, S = n_way * n_support support rows class-major, Q = n_way * n_query, M = episodes * Q):
//   zS, G, dG        [episodes, S, D]          encoder gates / h / c  [2 directions, episodes, S, 4D | D | D]
//   FCE h, c         [slots, M, D]             FCE gates [slots, M, 4D], attention a [slots, M, S], read r [slots, M, D]
#include "mft_common.h"

namespace {

constexpr int MN_D = 512;
constexpr int MN_MAX_S = 256;
constexpr int MN_MAX_WAY = 32;
constexpr int MN_SJ = MN_MAX_S / 64;          // support columns per lane
constexpr float MN_EPS = 1e-5f;

// ------------------------------------------------------------------------------------------------ fp32 GEMM
// c[z] = c_in[z] + bias1 + bias2 + op(a1[z]) op(b1[z]) + op(a2[z]) op(b2[z]);  op(a) is [M, K], op(b) is [K, N].
constexpr int GT = 64;            // output tile (GT x GT), 4 x 4 per thread
constexpr int GK = 16;            // k slice
constexpr int GFOLD = 8;          // slices per first-level partial sum (a power of two)

struct GemmPair {
    const float* a; const float* b; const float* b_alt;
    long long a_bs, b_bs;
    int lda, ldb, K;
};
struct GemmArgs {
    GemmPair p[2];
    const float* c_in; const float* bias1; const float* bias2; float* c;
    long long ci_bs, c_bs;
    int ldci, ldc, M, N;
};

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void mn_gemm_kernel(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[GK][GT + 4];
    __shared__ __attribute__((aligned(16))) float Bs[GK][GT + 4];
    const int z = blockIdx.z;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    // two-level sum: every GFOLD slices (128 k) the running partial sums are folded into `tot`, so the rounding error of a sum over
    // thousands of rows (the weight gradients) grows with sqrt(128) + sqrt(K / 128) instead of sqrt(K); the order stays fixed
    float acc[4][4], tot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j] = 0.f;
    for (int pi = 0; pi < 2; ++pi) {
        const GemmPair p = g.p[pi];
        if (p.a == nullptr || p.K <= 0) continue;
        const float* A = p.a + (long long)z * p.a_bs;
        const float* B = p.b_alt != nullptr ? ((z & 1) ? p.b_alt : p.b) : p.b + (long long)z * p.b_bs;
        float ra[4], rb[4];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = threadIdx.x + 256 * i;
                const int ka = TA ? idx >> 6 : idx & 15, ma = TA ? idx & 63 : idx >> 4;
                const bool oka = (k0 + ka < p.K) && (m0 + ma < g.M);
                ra[i] = oka ? (TA ? A[(long long)(k0 + ka) * p.lda + m0 + ma] : A[(long long)(m0 + ma) * p.lda + k0 + ka]) : 0.f;
                const int kb = TB ? idx & 15 : idx >> 6, nb = TB ? idx >> 4 : idx & 63;
                const bool okb = (k0 + kb < p.K) && (n0 + nb < g.N);
                rb[i] = okb ? (TB ? B[(long long)(n0 + nb) * p.ldb + k0 + kb] : B[(long long)(k0 + kb) * p.ldb + n0 + nb]) : 0.f;
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < p.K; k0 += GK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = threadIdx.x + 256 * i;
                As[TA ? idx >> 6 : idx & 15][TA ? idx & 63 : idx >> 4] = ra[i];
                Bs[TB ? idx & 15 : idx >> 6][TB ? idx >> 4 : idx & 63] = rb[i];
            }
            __syncthreads();
            if (k0 + GK < p.K) fetch(k0 + GK);            // the next slice travels while this one is multiplied
#pragma unroll
            for (int kk = 0; kk < GK; ++kk) {
                const f32x4 av = *(const f32x4*)&As[kk][ty * 4];
                const f32x4 bv = *(const f32x4*)&Bs[kk][tx * 4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
            }
            __syncthreads();
            if (((k0 / GK) & (GFOLD - 1)) == GFOLD - 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = 0.f; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += tot[i][j];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= g.N) continue;
            float v = acc[i][j];
            if (g.c_in) v += g.c_in[(long long)z * g.ci_bs + (long long)m * g.ldci + n];
            if (g.bias1) v += g.bias1[n];
            if (g.bias2) v += g.bias2[n];
            g.c[(long long)z * g.c_bs + (long long)m * g.ldc + n] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ LSTM cell (pointwise part)
__device__ __forceinline__ float mn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

struct LstmFwd {
    float* gates; const float* c_prev; const float* f_add; float* c_out; float* h_out;
    long long bs_g, bs_cp, bs_o;
    int ld_g, ld_cp, ld_f, ld_o, rows;
};

// gates [rows, 4D] hold the pre-activations (i, f, g, o) and leave with the activations; c' = f c + i g, h' = o tanh(c') (+ f_add)
__global__ __launch_bounds__(256) void mn_lstm_fwd_kernel(const LstmFwd a) {
    const int z = blockIdx.y;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.rows * MN_D) return;
    const int m = (int)(idx / MN_D), j = (int)(idx - (long long)m * MN_D);
    float* g = a.gates + z * a.bs_g + (long long)m * a.ld_g + j;
    const float gi = mn_sigmoid(g[0]), gf = mn_sigmoid(g[MN_D]), gg = tanhf(g[2 * MN_D]), go = mn_sigmoid(g[3 * MN_D]);
    const float cp = a.c_prev ? a.c_prev[z * a.bs_cp + (long long)m * a.ld_cp + j] : 0.f;
    const float c = gf * cp + gi * gg;
    float h = go * tanhf(c);
    if (a.f_add) h += a.f_add[(long long)m * a.ld_f + j];
    g[0] = gi; g[MN_D] = gf; g[2 * MN_D] = gg; g[3 * MN_D] = go;
    const long long o = z * a.bs_o + (long long)m * a.ld_o + j;
    a.c_out[o] = c;
    a.h_out[o] = h;
}

struct LstmBwd {
    float* gates; const float* c_prev; const float* c_new; const float* dh1; const float* dh2; const float* dc_in; float* dc_out;
    float* dh_sum; float* dgate_sum;
    long long bs_g, bs_cp, bs_cn, bs_d1, bs_d2, bs_dc;
    int ld_g, ld_cp, ld_cn, ld_d1, ld_d2, ld_dc, rows, accumulate;
};

// gates [rows, 4D] hold the activations and leave with d(pre-activations); dc_out = d(c_prev).  dh_sum (nullable, [rows, D])
// (+)= dh: the FCE's "h' += f" branch; dgate_sum (nullable, [rows, 4D]) (+)= d(pre-activations): the step-independent input part.
__global__ __launch_bounds__(256) void mn_lstm_bwd_kernel(const LstmBwd a) {
    const int z = blockIdx.y;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.rows * MN_D) return;
    const int m = (int)(idx / MN_D), j = (int)(idx - (long long)m * MN_D);
    float* g = a.gates + z * a.bs_g + (long long)m * a.ld_g + j;
    float dh = a.dh1[z * a.bs_d1 + (long long)m * a.ld_d1 + j];
    if (a.dh2) dh += a.dh2[z * a.bs_d2 + (long long)m * a.ld_d2 + j];
    const float gi = g[0], gf = g[MN_D], gg = g[2 * MN_D], go = g[3 * MN_D];
    const float cp = a.c_prev ? a.c_prev[z * a.bs_cp + (long long)m * a.ld_cp + j] : 0.f;
    const float tc = tanhf(a.c_new[z * a.bs_cn + (long long)m * a.ld_cn + j]);
    const long long od = z * a.bs_dc + (long long)m * a.ld_dc + j;
    float dc = dh * go * (1.f - tc * tc);
    if (a.dc_in) dc += a.dc_in[od];
    const float di = dc * gg * gi * (1.f - gi);
    const float df = dc * cp * gf * (1.f - gf);
    const float dg = dc * gi * (1.f - gg * gg);
    const float dO = dh * tc * go * (1.f - go);
    g[0] = di; g[MN_D] = df; g[2 * MN_D] = dg; g[3 * MN_D] = dO;
    a.dc_out[od] = dc * gf;
    if (a.dh_sum) {
        float* p = a.dh_sum + (long long)m * MN_D + j;
        *p = a.accumulate ? *p + dh : dh;
    }
    if (a.dgate_sum) {
        float* p = a.dgate_sum + (long long)m * 4 * MN_D + j;
        if (a.accumulate) { p[0] += di; p[MN_D] += df; p[2 * MN_D] += dg; p[3 * MN_D] += dO; }
        else { p[0] = di; p[MN_D] = df; p[2 * MN_D] = dg; p[3 * MN_D] = dO; }
    }
}

// ------------------------------------------------------------------------------------------------ rows in and out of the episode layout
struct MnShape {
    int episodes, n_way, ns, nq;
};

// feats [episodes, n_way, ns + nq, D] (row stride ld) -> zS [episodes, S, D], zQ [episodes * Q, D] (and h0, the FCE's first state)
__global__ __launch_bounds__(256) void mn_gather_kernel(const float* __restrict__ feats, int ld, MnShape s, float* __restrict__ zS,
                                                        float* __restrict__ zQ, float* __restrict__ h0) {
    const int per = s.ns + s.nq;
    const long long row = (long long)blockIdx.x * 2 + (threadIdx.x >> 7);
    if (row >= (long long)s.episodes * s.n_way * per) return;
    const int j = threadIdx.x & 127;
    const int i = (int)(row % per);
    const long long ec = row / per;                      // episode * n_way + class
    const f32x4 v = *(const f32x4*)(feats + row * ld + 4 * j);
    if (i < s.ns) {
        *(f32x4*)(zS + (ec * s.ns + i) * MN_D + 4 * j) = v;
    } else {
        const long long q = ec * s.nq + (i - s.ns);
        *(f32x4*)(zQ + q * MN_D + 4 * j) = v;
        if (h0) *(f32x4*)(h0 + q * MN_D + 4 * j) = v;
    }
}

// dfeats rows: support rows <- dzS, query rows <- dq1 (+ dq2)
__global__ __launch_bounds__(256) void mn_scatter_kernel(const float* __restrict__ dzS, const float* __restrict__ dq1,
                                                         const float* __restrict__ dq2, MnShape s, float* __restrict__ dfeats, int ldd) {
    const int per = s.ns + s.nq;
    const long long row = (long long)blockIdx.x * 2 + (threadIdx.x >> 7);
    if (row >= (long long)s.episodes * s.n_way * per) return;
    const int j = threadIdx.x & 127;
    const int i = (int)(row % per);
    const long long ec = row / per;
    f32x4 v;
    if (i < s.ns) {
        v = *(const f32x4*)(dzS + (ec * s.ns + i) * MN_D + 4 * j);
    } else {
        const long long q = ec * s.nq + (i - s.ns);
        v = *(const f32x4*)(dq1 + q * MN_D + 4 * j);
        if (dq2) v += *(const f32x4*)(dq2 + q * MN_D + 4 * j);
    }
    *(f32x4*)(dfeats + row * ldd + 4 * j) = v;
}

__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// G = zS + h_forward + h_reverse, gnorm = ||G||_2 per row; one wave per row
__global__ __launch_bounds__(256) void mn_combine_kernel(const float* __restrict__ zS, const float* __restrict__ hf,
                                                         const float* __restrict__ hr, long long rows, float* __restrict__ G,
                                                         float* __restrict__ gnorm) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long o = row * MN_D + 256 * i + 4 * lane;
        const f32x4 v = *(const f32x4*)(zS + o) + *(const f32x4*)(hf + o) + *(const f32x4*)(hr + o);
        *(f32x4*)(G + o) = v;
        ss += dot4(v, v);
    }
    ss = wave_sum(ss);
    if (lane == 0) gnorm[row] = sqrtf(ss);
}

// out[c] = sum_r x[r][c], rows in order; one thread per column
__global__ __launch_bounds__(256) void mn_colsum_kernel(const float* __restrict__ x, int ldx, int C, long long rows,
                                                        float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float acc = 0.f;
    for (long long r = 0; r < rows; ++r) acc += x[r * ldx + c];
    out[c] = acc;
}

// ------------------------------------------------------------------------------------------------ attention read of the FCE
// One wave per query row: a lane holds 8 of the row's 512 features and the support columns lane, lane + 64, ...
struct RowVec {
    f32x4 v0, v1;
};
__device__ __forceinline__ RowVec load_row(const float* p, int lane) {
    RowVec r;
    r.v0 = *(const f32x4*)(p + 4 * lane);
    r.v1 = *(const f32x4*)(p + 256 + 4 * lane);
    return r;
}
__device__ __forceinline__ void store_row(float* p, int lane, const RowVec r) {
    *(f32x4*)(p + 4 * lane) = r.v0;
    *(f32x4*)(p + 256 + 4 * lane) = r.v1;
}
__device__ __forceinline__ float row_dot(const RowVec a, const RowVec b) { return wave_sum(dot4(a.v0, b.v0) + dot4(a.v1, b.v1)); }

// col[j] of lane l <- x . G[s] for s = l + 64 j
__device__ __forceinline__ void row_times_Gt(const RowVec x, const float* __restrict__ Gp, int S, int lane, float col[MN_SJ]) {
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        col[j] = 0.f;
        for (int l = 0; l < 64 && 64 * j + l < S; ++l) {
            const float t = row_dot(x, load_row(Gp + (long long)(64 * j + l) * MN_D, lane));
            if (l == lane) col[j] = t;
        }
    }
}
// sum_s w_s * col_s G[s], w_s optional per-column weights [S]
__device__ __forceinline__ RowVec cols_times_G(const float col[MN_SJ], const float* __restrict__ Gp, int S, int lane) {
    RowVec r;
    r.v0 = (f32x4){0.f, 0.f, 0.f, 0.f};
    r.v1 = r.v0;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        for (int l = 0; l < 64 && 64 * j + l < S; ++l) {
            const float w = __shfl(col[j], l, 64);
            const RowVec gv = load_row(Gp + (long long)(64 * j + l) * MN_D, lane);
            r.v0 += w * gv.v0;
            r.v1 += w * gv.v1;
        }
    }
    return r;
}
// softmax over the S columns held as col[j] of lane l (s = l + 64 j)
__device__ __forceinline__ void softmax_cols(float col[MN_SJ], int S, int lane) {
    float mx = -3.4e38f;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) if (lane + 64 * j < S) mx = fmaxf(mx, col[j]);
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        col[j] = lane + 64 * j < S ? expf(col[j] - mx) : 0.f;
        se += col[j];
    }
    se = wave_sum(se);
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) col[j] = col[j] / se;
}

// a = softmax(h G^T) over the S columns, r = a G
__global__ __launch_bounds__(256) void mn_attention_fwd_kernel(const float* __restrict__ h, const float* __restrict__ G, int rows,
                                                               int Q, int S, float* __restrict__ a, float* __restrict__ r) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    const float* Gp = G + (long long)(m / Q) * S * MN_D;
    const RowVec hv = load_row(h + (long long)m * MN_D, lane);
    float col[MN_SJ];
    row_times_Gt(hv, Gp, S, lane, col);
    softmax_cols(col, S, lane);
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) if (lane + 64 * j < S) a[(long long)m * S + lane + 64 * j] = col[j];
    store_row(r + (long long)m * MN_D, lane, cols_times_G(col, Gp, S, lane));
}

// da = dr G^T, dlogit = a (da - sum a da), dh_out = dh_in + dlogit G.  (dG += a^T dr + dlogit^T h is a GEMM of the caller's.)
__global__ __launch_bounds__(256) void mn_attention_bwd_kernel(const float* __restrict__ dr, const float* __restrict__ a,
                                                               const float* __restrict__ G, const float* __restrict__ dh_in, int rows,
                                                               int Q, int S, float* __restrict__ dlogit, float* __restrict__ dh_out) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    const float* Gp = G + (long long)(m / Q) * S * MN_D;
    const RowVec dv = load_row(dr + (long long)m * MN_D, lane);
    float col[MN_SJ], av[MN_SJ];
    row_times_Gt(dv, Gp, S, lane, col);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        av[j] = lane + 64 * j < S ? a[(long long)m * S + lane + 64 * j] : 0.f;
        dot += av[j] * col[j];
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        col[j] = av[j] * (col[j] - dot);
        if (lane + 64 * j < S) dlogit[(long long)m * S + lane + 64 * j] = col[j];
    }
    RowVec o = cols_times_G(col, Gp, S, lane);
    if (dh_in) {
        const RowVec p = load_row(dh_in + (long long)m * MN_D, lane);
        o.v0 += p.v0;
        o.v1 += p.v1;
    }
    store_row(dh_out + (long long)m * MN_D, lane, o);
}

// ------------------------------------------------------------------------------------------------ read-out
// cos = (h . G_s) / ((||h|| + eps)(||G_s|| + eps)), p = softmax_s(100 relu(cos)), pc = class sums, logp = log(pc + 1e-6).
// The x100 in front of the softmax turns one fp32 rounding of a score near 85 (7.6e-6) into the same absolute error of a
// log-probability, so dot products, norms, cosines and the softmax are carried in double here (forward and backward); inputs and
// outputs stay fp32.  The kernels run once per step on a few hundred rows.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double dot8_d(const RowVec a, const RowVec b) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += (double)a.v0[i] * (double)b.v0[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) s += (double)a.v1[i] * (double)b.v1[i];
    return s;
}
struct RowVecD {
    double v[8];
};
__device__ __forceinline__ void axpy_d(RowVecD& acc, double w, const RowVec x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc.v[i] += w * (double)x.v0[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc.v[4 + i] += w * (double)x.v1[i];
}
__device__ __forceinline__ double dot_dv(const RowVecD a, const RowVec b) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += a.v[i] * (double)b.v0[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) s += a.v[4 + i] * (double)b.v1[i];
    return s;
}
// out = k1 * acc - k2 * x, rounded to fp32 once
__device__ __forceinline__ RowVec through_norm(const RowVecD acc, const RowVec x, double k1, double k2) {
    RowVec o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.v0[i] = (float)(k1 * acc.v[i] - k2 * (double)x.v0[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) o.v1[i] = (float)(k1 * acc.v[4 + i] - k2 * (double)x.v1[i]);
    return o;
}

__global__ __launch_bounds__(256) void mn_readout_fwd_kernel(const float* __restrict__ h, const float* __restrict__ G,
                                                             const float* __restrict__ gnorm, int rows, int Q, int S, int n_way, int ns,
                                                             float* __restrict__ cosv, float* __restrict__ p, float* __restrict__ hnorm,
                                                             float* __restrict__ pc, float* __restrict__ logp) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    const int e = m / Q;
    const float* Gp = G + (long long)e * S * MN_D;
    const RowVec hv = load_row(h + (long long)m * MN_D, lane);
    const double hn = sqrt(wave_sum_d(dot8_d(hv, hv)));
    double col[MN_SJ];
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        col[j] = 0.0;
        for (int l = 0; l < 64 && 64 * j + l < S; ++l) {
            const RowVec gv = load_row(Gp + (long long)(64 * j + l) * MN_D, lane);
            const double dot = wave_sum_d(dot8_d(hv, gv));
            const double gn = sqrt(wave_sum_d(dot8_d(gv, gv)));          // (the row's own norm in double; gnorm is its fp32 copy)
            if (l == lane) col[j] = dot / ((hn + (double)MN_EPS) * (gn + (double)MN_EPS));
        }
    }
    double mx = -1.0;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        const int s = lane + 64 * j;
        if (s < S) {
            cosv[(long long)m * S + s] = (float)col[j];
            col[j] = 100.0 * fmax(col[j], 0.0);
            mx = fmax(mx, col[j]);
        }
    }
    mx = wave_max_d(mx);
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        col[j] = lane + 64 * j < S ? exp(col[j] - mx) : 0.0;
        se += col[j];
    }
    se = wave_sum_d(se);
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        col[j] = col[j] / se;
        if (lane + 64 * j < S) p[(long long)m * S + lane + 64 * j] = (float)col[j];
    }
    if (lane == 0) hnorm[m] = (float)hn;
    for (int c = 0; c < n_way; ++c) {                      // class c owns the support columns [c ns, (c + 1) ns)
        double part = 0.0;
#pragma unroll
        for (int j = 0; j < MN_SJ; ++j) {
            const int s = lane + 64 * j;
            if (s >= c * ns && s < (c + 1) * ns) part += col[j];
        }
        part = wave_sum_d(part);
        if (lane == 0) {
            pc[(long long)m * n_way + c] = (float)part;
            logp[(long long)m * n_way + c] = (float)log(part + 1e-6);
        }
    }
}

// query side: dcos [rows, S] and dh through F^ = h / (||h|| + eps)
__global__ __launch_bounds__(256) void mn_readout_bwd_q_kernel(const float* __restrict__ dlogp, int ldg, const float* __restrict__ h,
                                                               const float* __restrict__ G, const float* __restrict__ gnorm,
                                                               const float* __restrict__ cosv, const float* __restrict__ p,
                                                               const float* __restrict__ hnorm, const float* __restrict__ pc, int rows,
                                                               int Q, int S, int n_way, int ns, float* __restrict__ dcos,
                                                               float* __restrict__ dh) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    const int e = m / Q;
    const float* Gp = G + (long long)e * S * MN_D;
    double pv[MN_SJ], dp[MN_SJ], col[MN_SJ];
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        const int s = lane + 64 * j;
        pv[j] = dp[j] = 0.0;
        if (s < S) {
            const int c = s / ns;
            pv[j] = (double)p[(long long)m * S + s];
            dp[j] = (double)dlogp[(long long)m * ldg + c] / ((double)pc[(long long)m * n_way + c] + 1e-6);
        }
        dot += pv[j] * dp[j];
    }
    dot = wave_sum_d(dot);
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j) {
        const int s = lane + 64 * j;
        col[j] = 0.0;
        if (s < S) {
            const double d = cosv[(long long)m * S + s] > 0.f ? 100.0 * pv[j] * (dp[j] - dot) : 0.0;
            dcos[(long long)m * S + s] = (float)d;
            col[j] = d / ((double)gnorm[(long long)e * S + s] + (double)MN_EPS);             // u = sum_s dcos_s G^_s
        }
    }
    RowVecD u;
#pragma unroll
    for (int i = 0; i < 8; ++i) u.v[i] = 0.0;
#pragma unroll
    for (int j = 0; j < MN_SJ; ++j)
        for (int l = 0; l < 64 && 64 * j + l < S; ++l)
            axpy_d(u, __shfl(col[j], l, 64), load_row(Gp + (long long)(64 * j + l) * MN_D, lane));
    const RowVec hv = load_row(h + (long long)m * MN_D, lane);
    const double hn = (double)hnorm[m];
    const double hu = wave_sum_d(dot_dv(u, hv));
    const double k1 = 1.0 / (hn + (double)MN_EPS);
    const double k2 = hn > 0.0 ? hu / (hn * (hn + (double)MN_EPS) * (hn + (double)MN_EPS)) : 0.0;
    store_row(dh + (long long)m * MN_D, lane, through_norm(u, hv, k1, k2));
}

// support side: v = sum_q dcos[q, s] F^_q (query rows in order), dG_s through G^ = G / (||G|| + eps); one wave per support row
__global__ __launch_bounds__(256) void mn_readout_bwd_s_kernel(const float* __restrict__ dcos, const float* __restrict__ h,
                                                               const float* __restrict__ hnorm, const float* __restrict__ G,
                                                               const float* __restrict__ gnorm, int episodes, int Q, int S,
                                                               float* __restrict__ dG) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= episodes * S) return;
    const int e = row / S, s = row - e * S;
    RowVecD v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v.v[i] = 0.0;
    for (int q = 0; q < Q; ++q) {
        const long long m = (long long)e * Q + q;
        axpy_d(v, (double)dcos[m * S + s] / ((double)hnorm[m] + (double)MN_EPS), load_row(h + m * MN_D, lane));
    }
    const RowVec gv = load_row(G + (long long)row * MN_D, lane);
    const double gn = (double)gnorm[row];
    const double gu = wave_sum_d(dot_dv(v, gv));
    const double k1 = 1.0 / (gn + (double)MN_EPS);
    const double k2 = gn > 0.0 ? gu / (gn * (gn + (double)MN_EPS) * (gn + (double)MN_EPS)) : 0.0;
    store_row(dG + (long long)row * MN_D, lane, through_norm(v, gv, k1, k2));
}

// ------------------------------------------------------------------------------------------------ NLL
__device__ __forceinline__ long long mn_label(const void* labels, int i64, int row) {
    return i64 ? ((const long long*)labels)[row] : (long long)((const int*)labels)[row];
}

__global__ __launch_bounds__(256) void mn_nll_mean_kernel(const float* __restrict__ logp, int ld, const void* __restrict__ labels,
                                                          int i64, int C, int rows, float* __restrict__ loss, double* loss_sum) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int row = threadIdx.x; row < rows; row += 256) {
        const long long y = mn_label(labels, i64, row);
        acc -= (y >= 0 && y < C) ? logp[(long long)row * ld + y] : __builtin_nanf("");
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {     // fixed tree: rerun- and replay-identical
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float l = part[0] / (float)rows;
        loss[0] = l;
        if (loss_sum) *loss_sum += (double)l;
    }
}

__global__ __launch_bounds__(256) void mn_nll_mean_bwd_kernel(const void* __restrict__ labels, int i64, int C, int rows,
                                                              const float* __restrict__ gout, float* __restrict__ dlogp, int ldd) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * C) return;
    const int row = (int)(idx / C), c = (int)(idx - (long long)row * C);
    const float g = (gout ? gout[0] : 1.f) / (float)rows;
    dlogp[(long long)row * ldd + c] = mn_label(labels, i64, row) == c ? -g : 0.f;
}

bool mn_shape_ok(int episodes, int n_way, int n_support, int n_query, int D) {
    if (episodes < 1 || n_way < 1 || n_way > MN_MAX_WAY || n_support < 1 || n_query < 1 || D != MN_D) return false;
    return (long long)n_way * n_support <= MN_MAX_S && (long long)episodes * n_way * n_query <= (1 << 24);
}
bool mn_al16(const void* p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mft_mn_gemm(int transa, int transb, int M, int N, int batch, const float* a1, int lda1, long long a1_bs,
                           const float* b1, const float* b1_alt, int ldb1, long long b1_bs, int K1, const float* a2, int lda2,
                           long long a2_bs, const float* b2, int ldb2, long long b2_bs, int K2, const float* c_in, int ldci,
                           long long ci_bs, const float* bias1, const float* bias2, float* c, int ldc, long long c_bs, void* stream) {
    if (M < 1 || N < 1 || batch < 1 || batch > 65535 || c == nullptr || ldc < N || K1 < 0 || K2 < 0) return MFT_EINVAL;
    if (b1_alt != nullptr && batch > 2) return MFT_EINVAL;
    if (c_in != nullptr && ldci < N) return MFT_EINVAL;
    if (cdiv(M, GT) > 65535) return MFT_EINVAL;
    const int K[2] = {K1, K2}, lda[2] = {lda1, lda2}, ldb[2] = {ldb1, ldb2};
    const float* a[2] = {a1, a2};
    const float* b[2] = {b1, b2};
    for (int i = 0; i < 2; ++i) {
        if (K[i] == 0) continue;
        if (a[i] == nullptr || b[i] == nullptr) return MFT_EINVAL;
        if (lda[i] < (transa ? M : K[i]) || ldb[i] < (transb ? K[i] : N)) return MFT_EINVAL;
    }
    GemmArgs g;
    g.p[0] = {a1, b1, b1_alt, a1_bs, b1_bs, lda1, ldb1, K1};
    g.p[1] = {a2, b2, nullptr, a2_bs, b2_bs, lda2, ldb2, K2};
    g.c_in = c_in; g.bias1 = bias1; g.bias2 = bias2; g.c = c;
    g.ci_bs = ci_bs; g.c_bs = c_bs; g.ldci = ldci; g.ldc = ldc; g.M = M; g.N = N;
    const dim3 grid(cdiv(N, GT), cdiv(M, GT), batch);
    hipStream_t st = (hipStream_t)stream;
    if (transa && transb) hipLaunchKernelGGL((mn_gemm_kernel<true, true>), grid, dim3(256), 0, st, g);
    else if (transa) hipLaunchKernelGGL((mn_gemm_kernel<true, false>), grid, dim3(256), 0, st, g);
    else if (transb) hipLaunchKernelGGL((mn_gemm_kernel<false, true>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((mn_gemm_kernel<false, false>), grid, dim3(256), 0, st, g);
    return mft_launch_status();
}

extern "C" int mft_lstm_step_forward(float* gates, int ld_g, long long bs_g, const float* c_prev, int ld_cp, long long bs_cp,
                                     const float* f_add, int ld_f, float* c_out, float* h_out, int ld_o, long long bs_o, int rows,
                                     int D, int batch, void* stream) {
    if (gates == nullptr || c_out == nullptr || h_out == nullptr || rows < 1 || D != MN_D || batch < 1 || batch > 65535)
        return MFT_EINVAL;
    if (ld_g < 4 * D || ld_o < D || (c_prev != nullptr && ld_cp < D) || (f_add != nullptr && ld_f < D)) return MFT_EINVAL;
    LstmFwd a;
    a.gates = gates; a.c_prev = c_prev; a.f_add = f_add; a.c_out = c_out; a.h_out = h_out;
    a.bs_g = bs_g; a.bs_cp = bs_cp; a.bs_o = bs_o;
    a.ld_g = ld_g; a.ld_cp = ld_cp; a.ld_f = ld_f; a.ld_o = ld_o; a.rows = rows;
    hipLaunchKernelGGL(mn_lstm_fwd_kernel, dim3(cdiv((long long)rows * D, 256), batch), dim3(256), 0, (hipStream_t)stream, a);
    return mft_launch_status();
}

extern "C" int mft_lstm_step_backward(float* gates, int ld_g, long long bs_g, const float* c_prev, int ld_cp, long long bs_cp,
                                      const float* c_new, int ld_cn, long long bs_cn, const float* dh1, int ld_d1, long long bs_d1,
                                      const float* dh2, int ld_d2, long long bs_d2, const float* dc_in, float* dc_out, int ld_dc,
                                      long long bs_dc, float* dh_sum, float* dgate_sum, int accumulate, int rows, int D, int batch,
                                      void* stream) {
    if (gates == nullptr || c_new == nullptr || dh1 == nullptr || dc_out == nullptr || rows < 1 || D != MN_D || batch < 1 ||
        batch > 65535)
        return MFT_EINVAL;
    if (ld_g < 4 * D || ld_cn < D || ld_d1 < D || ld_dc < D || (c_prev != nullptr && ld_cp < D) || (dh2 != nullptr && ld_d2 < D))
        return MFT_EINVAL;
    if ((dh_sum != nullptr || dgate_sum != nullptr) && batch != 1) return MFT_EINVAL;
    LstmBwd a;
    a.gates = gates; a.c_prev = c_prev; a.c_new = c_new; a.dh1 = dh1; a.dh2 = dh2; a.dc_in = dc_in; a.dc_out = dc_out;
    a.dh_sum = dh_sum; a.dgate_sum = dgate_sum;
    a.bs_g = bs_g; a.bs_cp = bs_cp; a.bs_cn = bs_cn; a.bs_d1 = bs_d1; a.bs_d2 = bs_d2; a.bs_dc = bs_dc;
    a.ld_g = ld_g; a.ld_cp = ld_cp; a.ld_cn = ld_cn; a.ld_d1 = ld_d1; a.ld_d2 = ld_d2; a.ld_dc = ld_dc; a.rows = rows;
    a.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(mn_lstm_bwd_kernel, dim3(cdiv((long long)rows * D, 256), batch), dim3(256), 0, (hipStream_t)stream, a);
    return mft_launch_status();
}

extern "C" int mft_mn_gather(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, float* zS,
                             float* zQ, float* h0, void* stream) {
    if (!mn_shape_ok(episodes, n_way, n_support, n_query, D) || !mn_al16(feats) || !mn_al16(zS) || !mn_al16(zQ)) return MFT_EINVAL;
    if (ld < D || (ld & 3) != 0 || (h0 != nullptr && !mn_al16(h0))) return MFT_EINVAL;
    const MnShape s = {episodes, n_way, n_support, n_query};
    const long long rows = (long long)episodes * n_way * (n_support + n_query);
    hipLaunchKernelGGL(mn_gather_kernel, dim3(cdiv(rows, 2)), dim3(256), 0, (hipStream_t)stream, feats, ld, s, zS, zQ, h0);
    return mft_launch_status();
}

extern "C" int mft_mn_scatter_backward(const float* dzS, const float* dq1, const float* dq2, int episodes, int n_way, int n_support,
                                       int n_query, int D, float* dfeats, int ldd, void* stream) {
    if (!mn_shape_ok(episodes, n_way, n_support, n_query, D) || !mn_al16(dzS) || !mn_al16(dq1) || !mn_al16(dfeats)) return MFT_EINVAL;
    if (ldd < D || (ldd & 3) != 0 || (dq2 != nullptr && !mn_al16(dq2))) return MFT_EINVAL;
    const MnShape s = {episodes, n_way, n_support, n_query};
    const long long rows = (long long)episodes * n_way * (n_support + n_query);
    hipLaunchKernelGGL(mn_scatter_kernel, dim3(cdiv(rows, 2)), dim3(256), 0, (hipStream_t)stream, dzS, dq1, dq2, s, dfeats, ldd);
    return mft_launch_status();
}

extern "C" int mft_mn_encode_combine(const float* zS, const float* hf, const float* hr, int episodes, int S, int D, float* G,
                                     float* gnorm, void* stream) {
    if (episodes < 1 || S < 1 || S > MN_MAX_S || D != MN_D || !mn_al16(zS) || !mn_al16(hf) || !mn_al16(hr) || !mn_al16(G) ||
        gnorm == nullptr)
        return MFT_EINVAL;
    const long long rows = (long long)episodes * S;
    hipLaunchKernelGGL(mn_combine_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, zS, hf, hr, rows, G, gnorm);
    return mft_launch_status();
}

extern "C" int mft_mn_colsum(const float* x, int ldx, int C, long long rows, float* out, void* stream) {
    if (x == nullptr || out == nullptr || C < 1 || ldx < C || rows < 1) return MFT_EINVAL;
    hipLaunchKernelGGL(mn_colsum_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, C, rows, out);
    return mft_launch_status();
}

extern "C" int mft_mn_attention_forward(const float* h, const float* G, int episodes, int Q, int S, int D, float* a, float* r,
                                        void* stream) {
    if (episodes < 1 || Q < 1 || S < 1 || S > MN_MAX_S || D != MN_D || (long long)episodes * Q > (1 << 24)) return MFT_EINVAL;
    if (!mn_al16(h) || !mn_al16(G) || a == nullptr || !mn_al16(r)) return MFT_EINVAL;
    const int rows = episodes * Q;
    hipLaunchKernelGGL(mn_attention_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, h, G, rows, Q, S, a, r);
    return mft_launch_status();
}

extern "C" int mft_mn_attention_backward(const float* dr, const float* a, const float* G, const float* dh_in, int episodes, int Q,
                                         int S, int D, float* dlogit, float* dh_out, void* stream) {
    if (episodes < 1 || Q < 1 || S < 1 || S > MN_MAX_S || D != MN_D || (long long)episodes * Q > (1 << 24)) return MFT_EINVAL;
    if (!mn_al16(dr) || a == nullptr || !mn_al16(G) || dlogit == nullptr || !mn_al16(dh_out)) return MFT_EINVAL;
    if (dh_in != nullptr && !mn_al16(dh_in)) return MFT_EINVAL;
    const int rows = episodes * Q;
    hipLaunchKernelGGL(mn_attention_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, dr, a, G, dh_in, rows, Q, S,
                       dlogit, dh_out);
    return mft_launch_status();
}

extern "C" int mft_mn_readout_forward(const float* h, const float* G, const float* gnorm, int episodes, int n_way, int n_support,
                                      int n_query, int D, float* cosv, float* p, float* hnorm, float* pc, float* logp, void* stream) {
    if (!mn_shape_ok(episodes, n_way, n_support, n_query, D) || !mn_al16(h) || !mn_al16(G)) return MFT_EINVAL;
    if (gnorm == nullptr || cosv == nullptr || p == nullptr || hnorm == nullptr || pc == nullptr || logp == nullptr) return MFT_EINVAL;
    const int Q = n_way * n_query, rows = episodes * Q;
    hipLaunchKernelGGL(mn_readout_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, h, G, gnorm, rows, Q,
                       n_way * n_support, n_way, n_support, cosv, p, hnorm, pc, logp);
    return mft_launch_status();
}

extern "C" int mft_mn_readout_backward(const float* dlogp, int ldg, const float* h, const float* G, const float* gnorm,
                                       const float* cosv, const float* p, const float* hnorm, const float* pc, int episodes, int n_way,
                                       int n_support, int n_query, int D, float* dcos, float* dh, float* dG, void* stream) {
    if (!mn_shape_ok(episodes, n_way, n_support, n_query, D) || !mn_al16(h) || !mn_al16(G) || !mn_al16(dh) || !mn_al16(dG))
        return MFT_EINVAL;
    if (dlogp == nullptr || ldg < n_way || gnorm == nullptr || cosv == nullptr || p == nullptr || hnorm == nullptr || pc == nullptr ||
        dcos == nullptr)
        return MFT_EINVAL;
    const int Q = n_way * n_query, S = n_way * n_support, rows = episodes * Q;
    hipLaunchKernelGGL(mn_readout_bwd_q_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, dlogp, ldg, h, G, gnorm, cosv,
                       p, hnorm, pc, rows, Q, S, n_way, n_support, dcos, dh);
    hipLaunchKernelGGL(mn_readout_bwd_s_kernel, dim3(cdiv((long long)episodes * S, 4)), dim3(256), 0, (hipStream_t)stream, dcos, h,
                       hnorm, G, gnorm, episodes, Q, S, dG);
    return mft_launch_status();
}

extern "C" int mft_nll_mean(const float* logp, int ld, const void* labels, int labels_i64, int C, int rows, float* loss,
                            double* loss_sum, void* stream) {
    if (logp == nullptr || labels == nullptr || loss == nullptr || rows < 1 || C < 1 || ld < C) return MFT_EINVAL;
    hipLaunchKernelGGL(mn_nll_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logp, ld, labels, labels_i64, C, rows, loss,
                       loss_sum);
    return mft_launch_status();
}

extern "C" int mft_nll_mean_backward(const void* labels, int labels_i64, int C, int rows, const float* grad_loss, float* dlogp,
                                     int ldd, void* stream) {
    if (labels == nullptr || dlogp == nullptr || rows < 1 || C < 1 || ldd < C) return MFT_EINVAL;
    hipLaunchKernelGGL(mn_nll_mean_bwd_kernel, dim3(cdiv((long long)rows * C, 256)), dim3(256), 0, (hipStream_t)stream, labels,
                       labels_i64, C, rows, grad_loss, dlogp, ldd);
    return mft_launch_status();
}
