// FEAT head (Ye et al., CVPR 2020: embedding adaptation with a set-to-set function) forward and backward,
// every set of every episode of a step per launch.
//
//   q = X Wq^T, k = X Wk^T, v = X Wv^T    P = softmax_rows(q k^T / sqrt(D))    o = (m_att P) v
//   h = m_out (o Wfc^T + b_fc) + X        A(X) = LayerNorm(h) ln_w + ln_b
//   scores[q, c] = -|z_q - A(prototypes)_c|^2 / temperature
//   train mode: centre_c = mean_rows A(rows of class c), reg[r, c] = -|z_r - centre_c|^2 / temperature2
//
// TOKENS.  X [Ntok, D]: the NP = episodes * n_way prototypes (one set of n_way tokens per episode), then -- in train mode -- the
// episodes * n_way * T feature rows (one set of T = n_support + n_query tokens per class).  P, dS and m_att hold one [t, t] block per
// set, in that order.
//
// Storage is fp32; every sum, the exponential and the normalisations run in double inside the kernels and round once on the store.
// No atomics; every sum runs in a fixed order, so two launches on the same input are bit-identical and an episode's result does not
// depend on the episodes beside it.  No kernel waits for another workgroup and the trip count of every loop is a function of the
// shape arguments alone: a non-finite feature gives non-finite output and the launch returns.
#include "philox.h"

namespace {

constexpr int FEAT_D = 512;
constexpr int FEAT_MAX_WAY = 32;
constexpr int FEAT_MAX_T = 128;             // one wave holds a softmax row, two entries per lane
constexpr int FEAT_THREADS = 256;
constexpr int FEAT_DRAW_THREADS = 1024;
constexpr double FEAT_LN_EPS = 1e-5;
static_assert(FEAT_MAX_WAY <= FEAT_MAX_T, "an episode's prototypes are a set too");

struct FeatShape {
    int E, n_way, ns, nq, T, NP, Ntok;
};

struct FeatSet {
    int start, t;               // first token row and number of tokens
    long long poff;             // offset of the set's [t, t] block
};

__device__ __forceinline__ FeatSet set_of_token(const FeatShape s, int i) {
    FeatSet r;
    if (i < s.NP) {
        const int e = i / s.n_way;
        r.start = e * s.n_way;
        r.t = s.n_way;
        r.poff = (long long)e * s.n_way * s.n_way;
    } else {
        const int c = (i - s.NP) / s.T;
        r.start = s.NP + c * s.T;
        r.t = s.T;
        r.poff = (long long)s.E * s.n_way * s.n_way + (long long)c * s.T * s.T;
    }
    return r;
}

template <int LANES>
__device__ __forceinline__ double dsum(double v) {
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double dmax64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = (o > v || o != o) ? o : v;          // a NaN wins: it reaches every lane
    }
    return v;
}

__device__ __forceinline__ double ddot4(const f32x4 a, const f32x4 b) {
    return (double)a.x * (double)b.x + (double)a.y * (double)b.y + (double)a.z * (double)b.z + (double)a.w * (double)b.w;
}

// feats row (within the whole batch) of query r of the batch (class-major inside an episode)
__device__ __forceinline__ long long query_row(const FeatShape s, int r) {
    const int Q = s.n_way * s.nq;
    const int e = r / Q, rr = r - e * Q, c = rr / s.nq;
    return (long long)e * s.n_way * s.T + (long long)c * s.T + s.ns + (rr - c * s.nq);
}

// ---------------------------------------------------------------------------------------------------------------- tokens
// one token row per workgroup of 128 threads, one float4 column each
__global__ __launch_bounds__(128) void feat_tokens_kernel(const float* __restrict__ feats, int ld, FeatShape s, float* __restrict__ X) {
    const int i = blockIdx.x, j = 4 * threadIdx.x;
    f32x4 out;
    if (i < s.NP) {
        const float* src = feats + (long long)i * s.T * ld + j;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = 0; r < s.ns; ++r) {
            const f32x4 v = *(const f32x4*)(src + (long long)r * ld);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += (double)v[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = (float)(acc[q] / (double)s.ns);
    } else {
        out = *(const f32x4*)(feats + (long long)(i - s.NP) * ld + j);
    }
    *(f32x4*)(X + (long long)i * FEAT_D + j) = out;
}

// ---------------------------------------------------------------------------------------------------------------- products
// C[z][i, j] = bias[j] + add[i, j] + sum_seg sum_k A[z + seg](i, k) B[z + seg](j, k), 32 x 32 tiles, 2 x 2 entries per thread, double
// accumulation in the order seg, k.  Only one of (gridDim.z, nseg) is larger than 1.  Element (i, k) of A is A[i * sai + k * sak].
struct FeatMm {
    const float* A[3];
    const float* B[3];
    long long sai, sak, sbj, sbk;
    int M, N, K, nseg;
    const float* bias;
    const float* add;
    float* C;
    long long ldc, zc;
};

__global__ __launch_bounds__(FEAT_THREADS) void feat_mm_kernel(FeatMm a) {
    __shared__ float sa[32][33], sb[32][33];
    const int tid = threadIdx.x, z = blockIdx.z;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const int ty = tid >> 4, tx = tid & 15;
    const int lo = tid & 31, hi = tid >> 5;
    const bool a_k_fast = a.sak == 1, b_k_fast = a.sbk == 1;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int seg = 0; seg < a.nseg; ++seg) {
        const float* A = a.A[z + seg];
        const float* B = a.B[z + seg];
        for (int k0 = 0; k0 < a.K; k0 += 32) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ra = a_k_fast ? hi + 8 * q : lo, ka = a_k_fast ? lo : hi + 8 * q;
                const int rb = b_k_fast ? hi + 8 * q : lo, kb = b_k_fast ? lo : hi + 8 * q;
                sa[ra][ka] = (i0 + ra < a.M && k0 + ka < a.K) ? A[(long long)(i0 + ra) * a.sai + (long long)(k0 + ka) * a.sak] : 0.f;
                sb[rb][kb] = (j0 + rb < a.N && k0 + kb < a.K) ? B[(long long)(j0 + rb) * a.sbj + (long long)(k0 + kb) * a.sbk] : 0.f;
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
    }
    float* C = a.C + (long long)z * a.zc;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
            if (i < a.M && j < a.N) {
                double v = acc[p][q];
                if (a.bias) v += (double)a.bias[j];
                if (a.add) v += (double)a.add[(long long)i * a.ldc + j];
                C[(long long)i * a.ldc + j] = (float)v;
            }
        }
}

int launch_mm(const FeatMm& a, int batch, hipStream_t stream) {
    hipLaunchKernelGGL(feat_mm_kernel, dim3(cdiv(a.N, 32), cdiv(a.M, 32), batch), dim3(FEAT_THREADS), 0, stream, a);
    return mft_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- attention
// one workgroup per token row i: the t scaled products q_i . k_j (a wave per j), the row softmax by wave 0, then o_i = sum_j
// (m_ij P_ij) v_j with two columns per thread, j in order.  The first term starts the sum, so t = 1 gives o = 1 * v = v.
__global__ __launch_bounds__(FEAT_THREADS) void feat_attention_kernel(const float* __restrict__ qkv, FeatShape s,
                                                                      const float* __restrict__ m_att, float* __restrict__ P,
                                                                      float* __restrict__ o) {
    __shared__ double sp[FEAT_MAX_T];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FeatSet st = set_of_token(s, i);
    const int r = i - st.start;
    const long long plane = (long long)s.Ntok * FEAT_D;
    const float* q = qkv + (long long)i * FEAT_D;
    const float* k = qkv + plane + (long long)st.start * FEAT_D;
    const float* v = qkv + 2 * plane + (long long)st.start * FEAT_D;
    const f32x4 q0 = *(const f32x4*)(q + 4 * lane), q1 = *(const f32x4*)(q + 256 + 4 * lane);
    const double scale = 1.0 / sqrt((double)FEAT_D);
    for (int j = wave; j < st.t; j += FEAT_THREADS / 64) {
        const float* kj = k + (long long)j * FEAT_D;
        const double d = dsum<64>(ddot4(q0, *(const f32x4*)(kj + 4 * lane)) + ddot4(q1, *(const f32x4*)(kj + 256 + 4 * lane)));
        if (lane == 0) sp[j] = d * scale;
    }
    __syncthreads();
    if (wave == 0) {
        const int ja = lane, jb = lane + 64;
        const bool la = ja < st.t, lb = jb < st.t;
        const double xa = la ? sp[ja] : 0.0, xb = lb ? sp[jb] : 0.0;
        double mx = la ? xa : -1.7976931348623157e308;
        if (lb && (xb > mx || xb != xb)) mx = xb;
        mx = dmax64(mx);
        const double ea = la ? exp(xa - mx) : 0.0, eb = lb ? exp(xb - mx) : 0.0;
        const double se = dsum<64>(ea + eb);
        const long long row = st.poff + (long long)r * st.t;
        if (la) {
            const double p = ea / se;
            P[row + ja] = (float)p;
            sp[ja] = m_att ? p * (double)m_att[row + ja] : p;
        }
        if (lb) {
            const double p = eb / se;
            P[row + jb] = (float)p;
            sp[jb] = m_att ? p * (double)m_att[row + jb] : p;
        }
    }
    __syncthreads();
    const int d0 = tid, d1 = tid + FEAT_THREADS;
    double a0 = sp[0] * (double)v[d0], a1 = sp[0] * (double)v[d1];
    for (int j = 1; j < st.t; ++j) {
        const double p = sp[j];
        a0 += p * (double)v[(long long)j * FEAT_D + d0];
        a1 += p * (double)v[(long long)j * FEAT_D + d1];
    }
    o[(long long)i * FEAT_D + d0] = (float)a0;
    o[(long long)i * FEAT_D + d1] = (float)a1;
}

// workgroup per token row i: dP_ij = m_ij (do_i . v_j), dS_ij = P_ij (dP_ij - sum_l dP_il P_il), dq_i = sum_j dS_ij k_j / sqrt(D)
__global__ __launch_bounds__(FEAT_THREADS) void feat_attention_bwd_rows_kernel(const float* __restrict__ d_o, const float* __restrict__ qkv,
                                                                               const float* __restrict__ P, const float* __restrict__ m_att,
                                                                               FeatShape s, float* __restrict__ dS, float* __restrict__ dqkv) {
    __shared__ double sp[FEAT_MAX_T];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FeatSet st = set_of_token(s, i);
    const int r = i - st.start;
    const long long plane = (long long)s.Ntok * FEAT_D;
    const float* g = d_o + (long long)i * FEAT_D;
    const float* k = qkv + plane + (long long)st.start * FEAT_D;
    const float* v = qkv + 2 * plane + (long long)st.start * FEAT_D;
    const long long row = st.poff + (long long)r * st.t;
    const f32x4 g0 = *(const f32x4*)(g + 4 * lane), g1 = *(const f32x4*)(g + 256 + 4 * lane);
    for (int j = wave; j < st.t; j += FEAT_THREADS / 64) {
        const float* vj = v + (long long)j * FEAT_D;
        const double d = dsum<64>(ddot4(g0, *(const f32x4*)(vj + 4 * lane)) + ddot4(g1, *(const f32x4*)(vj + 256 + 4 * lane)));
        if (lane == 0) sp[j] = m_att ? d * (double)m_att[row + j] : d;
    }
    __syncthreads();
    if (wave == 0) {
        const int ja = lane, jb = lane + 64;
        const bool la = ja < st.t, lb = jb < st.t;
        const double pa = la ? (double)P[row + ja] : 0.0, pb = lb ? (double)P[row + jb] : 0.0;
        const double ga = la ? sp[ja] : 0.0, gb = lb ? sp[jb] : 0.0;
        const double dot = dsum<64>(ga * pa + gb * pb);
        if (la) {
            const double t = pa * (ga - dot);
            dS[row + ja] = (float)t;
            sp[ja] = t;
        }
        if (lb) {
            const double t = pb * (gb - dot);
            dS[row + jb] = (float)t;
            sp[jb] = t;
        }
    }
    __syncthreads();
    const double scale = 1.0 / sqrt((double)FEAT_D);
    const int d0 = tid, d1 = tid + FEAT_THREADS;
    double a0 = 0.0, a1 = 0.0;
    for (int j = 0; j < st.t; ++j) {
        const double t = sp[j];
        a0 += t * (double)k[(long long)j * FEAT_D + d0];
        a1 += t * (double)k[(long long)j * FEAT_D + d1];
    }
    dqkv[(long long)i * FEAT_D + d0] = (float)(a0 * scale);
    dqkv[(long long)i * FEAT_D + d1] = (float)(a1 * scale);
}

// workgroup per token row j: dv_j = sum_i (m_ij P_ij) do_i, dk_j = sum_i dS_ij q_i / sqrt(D), i in order
__global__ __launch_bounds__(FEAT_THREADS) void feat_attention_bwd_cols_kernel(const float* __restrict__ d_o, const float* __restrict__ qkv,
                                                                               const float* __restrict__ P, const float* __restrict__ m_att,
                                                                               const float* __restrict__ dS, FeatShape s,
                                                                               float* __restrict__ dqkv) {
    __shared__ double sp[FEAT_MAX_T], sd[FEAT_MAX_T];
    const int jt = blockIdx.x, tid = threadIdx.x;
    const FeatSet st = set_of_token(s, jt);
    const int j = jt - st.start;
    const long long plane = (long long)s.Ntok * FEAT_D;
    if (tid < st.t) {
        const long long at = st.poff + (long long)tid * st.t + j;
        sp[tid] = m_att ? (double)P[at] * (double)m_att[at] : (double)P[at];
        sd[tid] = dS[at];
    }
    __syncthreads();
    const float* g = d_o + (long long)st.start * FEAT_D;
    const float* q = qkv + (long long)st.start * FEAT_D;
    const double scale = 1.0 / sqrt((double)FEAT_D);
    const int d0 = tid, d1 = tid + FEAT_THREADS;
    double v0 = 0.0, v1 = 0.0, k0 = 0.0, k1 = 0.0;
    for (int i = 0; i < st.t; ++i) {
        const double p = sp[i], t = sd[i];
        v0 += p * (double)g[(long long)i * FEAT_D + d0];
        v1 += p * (double)g[(long long)i * FEAT_D + d1];
        k0 += t * (double)q[(long long)i * FEAT_D + d0];
        k1 += t * (double)q[(long long)i * FEAT_D + d1];
    }
    float* dk = dqkv + plane + (long long)jt * FEAT_D;
    float* dv = dqkv + 2 * plane + (long long)jt * FEAT_D;
    dk[d0] = (float)(k0 * scale);
    dk[d1] = (float)(k1 * scale);
    dv[d0] = (float)v0;
    dv[d1] = (float)v1;
}

// ---------------------------------------------------------------------------------------------------------------- norm
// one wave per token row, eight columns per lane
struct FeatRow {
    double h[8];
};

__device__ __forceinline__ FeatRow load_h(const float* __restrict__ y, const float* __restrict__ X, const float* __restrict__ m_out,
                                          long long at, int lane) {
    FeatRow r;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long p = at + 256 * half + 4 * lane;
        const f32x4 yv = *(const f32x4*)(y + p), xv = *(const f32x4*)(X + p);
        const f32x4 one = {1.f, 1.f, 1.f, 1.f};
        const f32x4 mv = m_out ? *(const f32x4*)(m_out + p) : one;
#pragma unroll
        for (int q = 0; q < 4; ++q) r.h[4 * half + q] = (double)mv[q] * (double)yv[q] + (double)xv[q];
    }
    return r;
}

__global__ __launch_bounds__(FEAT_THREADS) void feat_norm_kernel(const float* __restrict__ y, const float* __restrict__ X,
                                                                 const float* __restrict__ m_out, const float* __restrict__ ln_w,
                                                                 const float* __restrict__ ln_b, int rows, float* __restrict__ A,
                                                                 float* __restrict__ mean, float* __restrict__ rstd) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * (FEAT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= rows) return;                                          // uniform over the wave
    const long long at = (long long)i * FEAT_D;
    const FeatRow r = load_h(y, X, m_out, at, lane);
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += r.h[q];
    const double mu = dsum<64>(sum) / (double)FEAT_D;
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) sq += (r.h[q] - mu) * (r.h[q] - mu);
    const double rs = 1.0 / sqrt(dsum<64>(sq) / (double)FEAT_D + FEAT_LN_EPS);
    if (lane == 0) {
        mean[i] = (float)mu;
        rstd[i] = (float)rs;
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int c = 256 * half + 4 * lane;
        const f32x4 w = *(const f32x4*)(ln_w + c), b = *(const f32x4*)(ln_b + c);
        f32x4 out;
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = (float)((r.h[4 * half + q] - mu) * rs * (double)w[q] + (double)b[q]);
        *(f32x4*)(A + at + c) = out;
    }
}

// dxh = dA ln_w, dh = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)); dy = m_out dh, dXres = dh
__global__ __launch_bounds__(FEAT_THREADS) void feat_norm_bwd_kernel(const float* __restrict__ dA, const float* __restrict__ y,
                                                                     const float* __restrict__ X, const float* __restrict__ m_out,
                                                                     const float* __restrict__ ln_w, const float* __restrict__ mean,
                                                                     const float* __restrict__ rstd, int rows, float* __restrict__ dy,
                                                                     float* __restrict__ dXres) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * (FEAT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= rows) return;
    const long long at = (long long)i * FEAT_D;
    const FeatRow r = load_h(y, X, m_out, at, lane);
    const double mu = mean[i], rs = rstd[i];
    double xh[8], dxh[8], s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int c = 256 * half + 4 * lane;
        const f32x4 w = *(const f32x4*)(ln_w + c), g = *(const f32x4*)(dA + at + c);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = 4 * half + q;
            xh[n] = (r.h[n] - mu) * rs;
            dxh[n] = (double)g[q] * (double)w[q];
            s1 += dxh[n];
            s2 += dxh[n] * xh[n];
        }
    }
    s1 = dsum<64>(s1) / (double)FEAT_D;
    s2 = dsum<64>(s2) / (double)FEAT_D;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long long p = at + 256 * half + 4 * lane;
        const f32x4 one = {1.f, 1.f, 1.f, 1.f};
        const f32x4 mv = m_out ? *(const f32x4*)(m_out + p) : one;
        f32x4 oy, ox;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = 4 * half + q;
            const double dh = rs * (dxh[n] - s1 - xh[n] * s2);
            ox[q] = (float)dh;
            oy[q] = (float)((double)mv[q] * dh);
        }
        *(f32x4*)(dy + p) = oy;
        *(f32x4*)(dXres + p) = ox;
    }
}

// column sums over the token rows: dln_w = sum dA xhat, dln_b = sum dA, db_fc = sum dy.  64 columns per workgroup; wave w sums the
// w-th quarter of the rows in row order, then the four quarters are added in order
__global__ __launch_bounds__(FEAT_THREADS) void feat_norm_colsum_kernel(const float* __restrict__ dA, const float* __restrict__ y,
                                                                        const float* __restrict__ X, const float* __restrict__ m_out,
                                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                        const float* __restrict__ dy, int rows, float* __restrict__ dln_w,
                                                                        float* __restrict__ dln_b, float* __restrict__ dbfc) {
    __shared__ double spart[FEAT_THREADS / 64][3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = blockIdx.x * 64 + lane;
    const int per = (rows + FEAT_THREADS / 64 - 1) / (FEAT_THREADS / 64);
    const int r1 = min(rows, (wave + 1) * per);
    double aw = 0.0, ab = 0.0, ay = 0.0;
    for (int i = wave * per; i < r1; ++i) {
        const long long p = (long long)i * FEAT_D + d;
        const double h = (m_out ? (double)m_out[p] : 1.0) * (double)y[p] + (double)X[p];
        const double xh = (h - (double)mean[i]) * (double)rstd[i];
        const double g = dA[p];
        aw += g * xh;
        ab += g;
        ay += (double)dy[p];
    }
    spart[wave][0][lane] = aw;
    spart[wave][1][lane] = ab;
    spart[wave][2][lane] = ay;
    __syncthreads();
    if (wave < 3) {
        const double v = ((spart[0][wave][lane] + spart[1][wave][lane]) + spart[2][wave][lane]) + spart[3][wave][lane];
        (wave == 0 ? dln_w : wave == 1 ? dln_b : dbfc)[d] = (float)v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- distances
// centre of class set c: the mean over its T adapted tokens, in row order; two columns per thread
__global__ __launch_bounds__(FEAT_THREADS) void feat_centre_kernel(const float* __restrict__ A, FeatShape s, float* __restrict__ centre) {
    const int c = blockIdx.x, d0 = threadIdx.x, d1 = threadIdx.x + FEAT_THREADS;
    const float* a = A + ((long long)s.NP + (long long)c * s.T) * FEAT_D;
    double v0 = 0.0, v1 = 0.0;
    for (int r = 0; r < s.T; ++r) {
        v0 += (double)a[(long long)r * FEAT_D + d0];
        v1 += (double)a[(long long)r * FEAT_D + d1];
    }
    centre[(long long)c * FEAT_D + d0] = (float)(v0 / (double)s.T);
    centre[(long long)c * FEAT_D + d1] = (float)(v1 / (double)s.T);
}

// out[r, c] = -|z_r - cen_c|^2 / temp, one wave per row.  all_rows = 0: the rows are the queries and cen the adapted prototypes;
// all_rows = 1: every feature row against the class centres
__global__ __launch_bounds__(FEAT_THREADS) void feat_dist_kernel(const float* __restrict__ feats, int ld, FeatShape s, int all_rows,
                                                                 const float* __restrict__ cen, float temp, int rows,
                                                                 float* __restrict__ out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (FEAT_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int per_ep = all_rows ? s.n_way * s.T : s.n_way * s.nq;
    const int e = r / per_ep;
    const float* z = feats + (all_rows ? (long long)r : query_row(s, r)) * ld;
    const float* ce = cen + (long long)e * s.n_way * FEAT_D;
    const f32x4 z0 = *(const f32x4*)(z + 4 * lane), z1 = *(const f32x4*)(z + 256 + 4 * lane);
    for (int c = 0; c < s.n_way; ++c) {
        const f32x4 p0 = *(const f32x4*)(ce + (long long)c * FEAT_D + 4 * lane), p1 = *(const f32x4*)(ce + (long long)c * FEAT_D + 256 + 4 * lane);
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double a = (double)z0[q] - (double)p0[q], b = (double)z1[q] - (double)p1[q];
            acc += a * a + b * b;
        }
        acc = dsum<64>(acc);
        if (lane == 0) out[(long long)r * s.n_way + c] = (float)(-acc / (double)temp);
    }
}

// one wave per feature row: ddirect = sum_c -2 g[q, c] (z - P'_c) / temp (a query row) + sum_c -2 greg[r, c] (z - centre_c) / temp2
// (train mode), the classes in order, the main term first; zero where there is neither
__global__ __launch_bounds__(FEAT_THREADS) void feat_dist_bwd_rows_kernel(const float* __restrict__ feats, int ld, FeatShape s, int train,
                                                                          const float* __restrict__ A, const float* __restrict__ centre,
                                                                          const float* __restrict__ dscores, const float* __restrict__ dreg,
                                                                          float temp, float temp2, int rows, float* __restrict__ ddirect) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (FEAT_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int per_ep = s.n_way * s.T;
    const int e = r / per_ep, rr = r - e * per_ep, cl = rr / s.T, pos = rr - cl * s.T;
    const float* z = feats + (long long)r * ld;
    double zz[8], acc[8];
    {
        const f32x4 z0 = *(const f32x4*)(z + 4 * lane), z1 = *(const f32x4*)(z + 256 + 4 * lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            zz[q] = z0[q];
            zz[4 + q] = z1[q];
            acc[q] = acc[4 + q] = 0.0;
        }
    }
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? pos < s.ns : !train) continue;              // uniform over the wave
        const float* cen = (pass == 0 ? A : centre) + (long long)e * s.n_way * FEAT_D;
        const float* g = pass == 0 ? dscores + ((long long)e * s.n_way * s.nq + (long long)cl * s.nq + (pos - s.ns)) * s.n_way
                                   : dreg + (long long)r * s.n_way;
        const double t = pass == 0 ? (double)temp : (double)temp2;
        for (int c = 0; c < s.n_way; ++c) {
            const double w = -2.0 * (double)g[c] / t;
            const f32x4 p0 = *(const f32x4*)(cen + (long long)c * FEAT_D + 4 * lane), p1 = *(const f32x4*)(cen + (long long)c * FEAT_D + 256 + 4 * lane);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[q] += w * (zz[q] - (double)p0[q]);
                acc[4 + q] += w * (zz[4 + q] - (double)p1[q]);
            }
        }
    }
    f32x4 o0, o1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o0[q] = (float)acc[q];
        o1[q] = (float)acc[4 + q];
    }
    *(f32x4*)(ddirect + (long long)r * FEAT_D + 4 * lane) = o0;
    *(f32x4*)(ddirect + (long long)r * FEAT_D + 256 + 4 * lane) = o1;
}

// one workgroup per (episode, class) and side (blockIdx.y: 0 = adapted prototype, 1 = class centre), two columns per thread:
// dcen_c = sum_rows 2 g[row, c] (z_row - cen_c) / temp in row order.  Side 0 writes the prototype token's dA, side 1 writes
// dcen_c / T to the T tokens of the class
__global__ __launch_bounds__(FEAT_THREADS) void feat_dist_bwd_centres_kernel(const float* __restrict__ feats, int ld, FeatShape s,
                                                                             const float* __restrict__ A, const float* __restrict__ centre,
                                                                             const float* __restrict__ dscores, const float* __restrict__ dreg,
                                                                             float temp, float temp2, float* __restrict__ dA) {
    const int ec = blockIdx.x, side = blockIdx.y, e = ec / s.n_way, c = ec - e * s.n_way;
    const int d0 = threadIdx.x, d1 = threadIdx.x + FEAT_THREADS;
    const float* cen = (side == 0 ? A : centre) + (long long)ec * FEAT_D;
    const double c0 = cen[d0], c1 = cen[d1];
    const int n = side == 0 ? s.n_way * s.nq : s.n_way * s.T;
    const float* g = side == 0 ? dscores + (long long)e * n * s.n_way : dreg + (long long)e * n * s.n_way;
    double a0 = 0.0, a1 = 0.0;
    for (int r = 0; r < n; ++r) {
        const float* z = feats + (side == 0 ? query_row(s, e * n + r) : (long long)e * n + r) * ld;
        const double w = g[(long long)r * s.n_way + c];
        a0 += w * ((double)z[d0] - c0);
        a1 += w * ((double)z[d1] - c1);
    }
    const double f = 2.0 / (side == 0 ? (double)temp : (double)temp2);
    if (side == 0) {
        dA[(long long)ec * FEAT_D + d0] = (float)(a0 * f);
        dA[(long long)ec * FEAT_D + d1] = (float)(a1 * f);
    } else {
        const float v0 = (float)(a0 * f / (double)s.T), v1 = (float)(a1 * f / (double)s.T);
        float* out = dA + ((long long)s.NP + (long long)ec * s.T) * FEAT_D;
        for (int r = 0; r < s.T; ++r) {
            out[(long long)r * FEAT_D + d0] = v0;
            out[(long long)r * FEAT_D + d1] = v1;
        }
    }
}

// every row of dfeats once: the direct term, the prototype's share for a support row, the row's own token in train mode
__global__ __launch_bounds__(128) void feat_dfeats_kernel(const float* __restrict__ ddirect, const float* __restrict__ dX, FeatShape s,
                                                          int train, float* __restrict__ dfeats, int ldd) {
    const int r = blockIdx.x, j = 4 * threadIdx.x;
    const int cls = r / s.T, pos = r - cls * s.T;                    // cls = episode * n_way + class: the prototype token
    const f32x4 a = *(const f32x4*)(ddirect + (long long)r * FEAT_D + j);
    double acc[4] = {a[0], a[1], a[2], a[3]};
    if (pos < s.ns) {
        const f32x4 p = *(const f32x4*)(dX + (long long)cls * FEAT_D + j);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += (double)p[q] / (double)s.ns;
    }
    if (train) {
        const f32x4 t = *(const f32x4*)(dX + ((long long)s.NP + r) * FEAT_D + j);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += (double)t[q];
    }
    const f32x4 out = {(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
    *(f32x4*)(dfeats + (long long)r * ldd + j) = out;
}

// ---------------------------------------------------------------------------------------------------------------- loss
// the cross entropy of row r (label y) of x [.., C], C <= 32
__device__ __forceinline__ double ce_row(const float* __restrict__ x, int C, int y) {
    double mx = (double)x[0];
    for (int c = 1; c < C; ++c) {
        const double v = x[c];
        mx = (v > mx || v != v) ? v : mx;
    }
    double se = 0.0;
    for (int c = 0; c < C; ++c) se += exp((double)x[c] - mx);
    return log(se) - ((double)x[y] - mx);
}

__device__ __forceinline__ double block_tree_sum(double* part, double v) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = FEAT_THREADS / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    const double r = part[0];
    __syncthreads();
    return r;
}

// one workgroup, a thread per row, a fixed tree over the threads.  The label of query row r is (r mod Q) / n_query, the label of
// feature row r is (r / T) mod n_way
__global__ __launch_bounds__(FEAT_THREADS) void feat_loss_kernel(const float* __restrict__ scores, const float* __restrict__ reg, FeatShape s,
                                                                 float balance, float* __restrict__ out, double* loss_sum) {
    __shared__ double part[FEAT_THREADS];
    const int Q = s.n_way * s.nq, rows_q = s.E * Q, rows_a = s.E * s.n_way * s.T;
    double acc = 0.0;
    for (int r = threadIdx.x; r < rows_q; r += FEAT_THREADS) acc += ce_row(scores + (long long)r * s.n_way, s.n_way, (r % Q) / s.nq);
    const double main_l = block_tree_sum(part, acc) / (double)rows_q;
    double aux_l = 0.0;
    if (reg) {
        acc = 0.0;
        for (int r = threadIdx.x; r < rows_a; r += FEAT_THREADS) acc += ce_row(reg + (long long)r * s.n_way, s.n_way, (r / s.T) % s.n_way);
        aux_l = block_tree_sum(part, acc) / (double)rows_a;
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(main_l + (double)balance * aux_l);
        out[1] = (float)main_l;
        out[2] = (float)aux_l;
        if (loss_sum) *loss_sum += (double)(float)main_l;
    }
}

// a thread per row of either matrix: d[r, c] = (softmax(x_r)[c] - [c == y_r]) * scale
__global__ __launch_bounds__(FEAT_THREADS) void feat_loss_bwd_kernel(const float* __restrict__ scores, const float* __restrict__ reg,
                                                                     FeatShape s, float balance, const float* __restrict__ gout,
                                                                     float* __restrict__ dscores, float* __restrict__ dreg) {
    const int Q = s.n_way * s.nq, rows_q = s.E * Q, rows_a = reg ? s.E * s.n_way * s.T : 0;
    const int r = blockIdx.x * FEAT_THREADS + threadIdx.x;
    if (r >= rows_q + rows_a) return;
    const bool aux = r >= rows_q;
    const int rr = aux ? r - rows_q : r;
    const float* x = (aux ? reg : scores) + (long long)rr * s.n_way;
    float* d = (aux ? dreg : dscores) + (long long)rr * s.n_way;
    const int y = aux ? (rr / s.T) % s.n_way : (rr % Q) / s.nq;
    const double g = gout ? (double)gout[0] : 1.0;
    const double sc = aux ? g * (double)balance / (double)rows_a : g / (double)rows_q;
    double mx = (double)x[0];
    for (int c = 1; c < s.n_way; ++c) {
        const double v = x[c];
        mx = (v > mx || v != v) ? v : mx;
    }
    double se = 0.0;
    for (int c = 0; c < s.n_way; ++c) se += exp((double)x[c] - mx);
    for (int c = 0; c < s.n_way; ++c) d[c] = (float)((exp((double)x[c] - mx) / se - (c == y ? 1.0 : 0.0)) * sc);
}

// ---------------------------------------------------------------------------------------------------------------- dropout draw
// ONE workgroup (the draw-index contract of fwt_draw_fold_kernel): every thread reads the index, then -- behind a barrier -- thread
// 0 stores index + 1
__device__ __forceinline__ float feat_multiplier(long long i, unsigned id, unsigned i2, unsigned i3, unsigned k0, unsigned k1, float p) {
    unsigned w0, w1;
    philox4x32_10((unsigned)i, (unsigned)((unsigned long long)i >> 32) | (id << 31), i2, i3, k0, k1, w0, w1);
    const bool keep = (double)w0 * (1.0 / 4294967296.0) >= (double)p;
    return keep ? (float)(1.0 / (1.0 - (double)p)) : 0.f;
}

__global__ __launch_bounds__(FEAT_DRAW_THREADS) void feat_draw_kernel(long long n_att, long long n_out, float p_att, float p_out,
                                                                      unsigned long long seed, unsigned long long* index,
                                                                      const float* __restrict__ in_att, const float* __restrict__ in_out,
                                                                      float* __restrict__ m_att, float* __restrict__ m_out) {
    const unsigned long long idx = *index;
    __syncthreads();                                   // every thread holds the index before thread 0 replaces it
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const unsigned i2 = (unsigned)idx, i3 = (unsigned)(idx >> 32);
    for (long long i = threadIdx.x; i < n_att; i += FEAT_DRAW_THREADS)
        m_att[i] = in_att ? in_att[i] : feat_multiplier(i, 0u, i2, i3, k0, k1, p_att);
    for (long long i = threadIdx.x; i < n_out; i += FEAT_DRAW_THREADS)
        m_out[i] = in_out ? in_out[i] : feat_multiplier(i, 1u, i2, i3, k0, k1, p_out);
    if (threadIdx.x == 0) *index = idx + 1;
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool feat_shape(int episodes, int n_way, int n_support, int n_query, int D, int train, FeatShape& s) {
    if (episodes < 1 || n_way < 1 || n_way > FEAT_MAX_WAY || n_support < 1 || n_query < 1 || D != FEAT_D) return false;
    const long long T = (long long)n_support + n_query;
    if (T > FEAT_MAX_T) return false;
    const long long NP = (long long)episodes * n_way, NA = NP * T, Ntok = NP + (train ? NA : 0);
    const long long blocks = NP * n_way + (train ? NA * T : 0);
    if ((NP + NA) * FEAT_D > 0x7fffffffLL || blocks > 0x7fffffffLL) return false;
    s = {episodes, n_way, n_support, n_query, (int)T, (int)NP, (int)Ntok};
    return true;
}

inline bool rows_ok(const void* p, int ld) { return p != nullptr && ld >= FEAT_D && (ld & 3) == 0 && ((uintptr_t)p & 15) == 0; }
inline bool al16(const void* p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mft_feat_tokens(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, int train,
                               float* X, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !rows_ok(feats, ld) || !al16(X)) return MFT_EINVAL;
    hipLaunchKernelGGL(feat_tokens_kernel, dim3(s.Ntok), dim3(128), 0, (hipStream_t)stream, feats, ld, s, X);
    return mft_launch_status();
}

extern "C" int mft_feat_project(const float* X, int episodes, int n_way, int n_support, int n_query, int D, int train, const float* wq,
                                const float* wk, const float* wv, float* qkv, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !X || !wq || !wk || !wv || !al16(qkv)) return MFT_EINVAL;
    FeatMm a = {};
    a.A[0] = a.A[1] = a.A[2] = X;
    a.B[0] = wq; a.B[1] = wk; a.B[2] = wv;
    a.sai = FEAT_D; a.sak = 1; a.sbj = FEAT_D; a.sbk = 1;
    a.M = s.Ntok; a.N = FEAT_D; a.K = FEAT_D; a.nseg = 1;
    a.C = qkv; a.ldc = FEAT_D; a.zc = (long long)s.Ntok * FEAT_D;
    return launch_mm(a, 3, (hipStream_t)stream);
}

extern "C" int mft_feat_attention(const float* qkv, int episodes, int n_way, int n_support, int n_query, int D, int train,
                                  const float* m_att, float* P, float* o, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !al16(qkv) || !P || !o) return MFT_EINVAL;
    hipLaunchKernelGGL(feat_attention_kernel, dim3(s.Ntok), dim3(FEAT_THREADS), 0, (hipStream_t)stream, qkv, s, m_att, P, o);
    return mft_launch_status();
}

extern "C" int mft_feat_fc(const float* o, int episodes, int n_way, int n_support, int n_query, int D, int train, const float* wfc,
                           const float* bfc, float* y, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !o || !wfc || !bfc || !y) return MFT_EINVAL;
    FeatMm a = {};
    a.A[0] = o; a.B[0] = wfc;
    a.sai = FEAT_D; a.sak = 1; a.sbj = FEAT_D; a.sbk = 1;
    a.M = s.Ntok; a.N = FEAT_D; a.K = FEAT_D; a.nseg = 1;
    a.bias = bfc; a.C = y; a.ldc = FEAT_D;
    return launch_mm(a, 1, (hipStream_t)stream);
}

extern "C" int mft_feat_norm(const float* y, const float* X, int episodes, int n_way, int n_support, int n_query, int D, int train,
                             const float* m_out, const float* ln_w, const float* ln_b, float* A, float* mean, float* rstd,
                             void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !al16(y) || !al16(X) || (m_out && !al16(m_out)) || !al16(ln_w) ||
        !al16(ln_b) || !al16(A) || !mean || !rstd)
        return MFT_EINVAL;
    hipLaunchKernelGGL(feat_norm_kernel, dim3(cdiv(s.Ntok, FEAT_THREADS / 64)), dim3(FEAT_THREADS), 0, (hipStream_t)stream, y, X, m_out,
                       ln_w, ln_b, s.Ntok, A, mean, rstd);
    return mft_launch_status();
}

extern "C" int mft_feat_scores(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, int train,
                               const float* A, float temperature, float temperature2, float* scores, float* centre, float* reg,
                               void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !rows_ok(feats, ld) || !al16(A) || !scores ||
        !(temperature > 0.f) || (train && (!al16(centre) || !reg || !(temperature2 > 0.f))))
        return MFT_EINVAL;
    const int rows_q = s.NP * s.nq;
    hipLaunchKernelGGL(feat_dist_kernel, dim3(cdiv(rows_q, FEAT_THREADS / 64)), dim3(FEAT_THREADS), 0, (hipStream_t)stream, feats, ld, s, 0,
                       A, temperature, rows_q, scores);
    if (train) {
        const int rows_a = s.NP * s.T;
        hipLaunchKernelGGL(feat_centre_kernel, dim3(s.NP), dim3(FEAT_THREADS), 0, (hipStream_t)stream, A, s, centre);
        hipLaunchKernelGGL(feat_dist_kernel, dim3(cdiv(rows_a, FEAT_THREADS / 64)), dim3(FEAT_THREADS), 0, (hipStream_t)stream, feats, ld,
                           s, 1, centre, temperature2, rows_a, reg);
    }
    return mft_launch_status();
}

extern "C" int mft_feat_loss(const float* scores, const float* reg, int episodes, int n_way, int n_support, int n_query, float balance,
                             float* out, double* loss_sum, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, FEAT_D, reg != nullptr, s) || !scores || !out) return MFT_EINVAL;
    hipLaunchKernelGGL(feat_loss_kernel, dim3(1), dim3(FEAT_THREADS), 0, (hipStream_t)stream, scores, reg, s, balance, out, loss_sum);
    return mft_launch_status();
}

extern "C" int mft_feat_loss_backward(const float* scores, const float* reg, int episodes, int n_way, int n_support, int n_query,
                                      float balance, const float* grad_loss, float* dscores, float* dreg, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, FEAT_D, reg != nullptr, s) || !scores || !dscores || (reg && !dreg))
        return MFT_EINVAL;
    const int rows = s.NP * s.nq + (reg ? s.NP * s.T : 0);
    hipLaunchKernelGGL(feat_loss_bwd_kernel, dim3(cdiv(rows, FEAT_THREADS)), dim3(FEAT_THREADS), 0, (hipStream_t)stream, scores, reg, s,
                       balance, grad_loss, dscores, dreg);
    return mft_launch_status();
}

extern "C" int mft_feat_scores_backward(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D, int train,
                                        const float* A, const float* centre, const float* dscores, const float* dreg, float temperature,
                                        float temperature2, float* ddirect, float* dA, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !rows_ok(feats, ld) || !al16(A) || !dscores || !al16(ddirect) ||
        !dA || !(temperature > 0.f) || (train && (!al16(centre) || !dreg || !(temperature2 > 0.f))))
        return MFT_EINVAL;
    const int rows = s.NP * s.T;
    hipLaunchKernelGGL(feat_dist_bwd_rows_kernel, dim3(cdiv(rows, FEAT_THREADS / 64)), dim3(FEAT_THREADS), 0, (hipStream_t)stream, feats, ld,
                       s, train ? 1 : 0, A, centre, dscores, dreg, temperature, temperature2, rows, ddirect);
    hipLaunchKernelGGL(feat_dist_bwd_centres_kernel, dim3(s.NP, train ? 2 : 1), dim3(FEAT_THREADS), 0, (hipStream_t)stream, feats, ld, s, A,
                       centre, dscores, dreg, temperature, temperature2, dA);
    return mft_launch_status();
}

extern "C" int mft_feat_norm_backward(const float* dA, const float* y, const float* X, int episodes, int n_way, int n_support,
                                      int n_query, int D, int train, const float* m_out, const float* ln_w, const float* mean,
                                      const float* rstd, float* dy, float* dXres, float* dln_w, float* dln_b, float* dbfc, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !al16(dA) || !al16(y) || !al16(X) || (m_out && !al16(m_out)) ||
        !al16(ln_w) || !mean || !rstd || !al16(dy) || !al16(dXres) || !dln_w || !dln_b || !dbfc)
        return MFT_EINVAL;
    hipLaunchKernelGGL(feat_norm_bwd_kernel, dim3(cdiv(s.Ntok, FEAT_THREADS / 64)), dim3(FEAT_THREADS), 0, (hipStream_t)stream, dA, y, X,
                       m_out, ln_w, mean, rstd, s.Ntok, dy, dXres);
    hipLaunchKernelGGL(feat_norm_colsum_kernel, dim3(FEAT_D / 64), dim3(FEAT_THREADS), 0, (hipStream_t)stream, dA, y, X, m_out, mean, rstd,
                       dy, s.Ntok, dln_w, dln_b, dbfc);
    return mft_launch_status();
}

extern "C" int mft_feat_fc_backward(const float* dy, const float* o, int episodes, int n_way, int n_support, int n_query, int D,
                                    int train, const float* wfc, float* d_o, float* dwfc, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !dy || !o || !wfc || !d_o || !dwfc) return MFT_EINVAL;
    FeatMm a = {};                                                  // do[r, k] = sum_n dy[r, n] Wfc[n, k]
    a.A[0] = dy; a.B[0] = wfc;
    a.sai = FEAT_D; a.sak = 1; a.sbj = 1; a.sbk = FEAT_D;
    a.M = s.Ntok; a.N = FEAT_D; a.K = FEAT_D; a.nseg = 1;
    a.C = d_o; a.ldc = FEAT_D;
    int rc = launch_mm(a, 1, (hipStream_t)stream);
    if (rc != 0) return rc;
    FeatMm b = {};                                                  // dWfc[n, k] = sum_r dy[r, n] o[r, k], r in order
    b.A[0] = dy; b.B[0] = o;
    b.sai = 1; b.sak = FEAT_D; b.sbj = 1; b.sbk = FEAT_D;
    b.M = FEAT_D; b.N = FEAT_D; b.K = s.Ntok; b.nseg = 1;
    b.C = dwfc; b.ldc = FEAT_D;
    return launch_mm(b, 1, (hipStream_t)stream);
}

extern "C" int mft_feat_attention_backward(const float* d_o, const float* qkv, const float* P, const float* m_att, int episodes, int n_way,
                                           int n_support, int n_query, int D, int train, float* dS, float* dqkv, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !al16(d_o) || !al16(qkv) || !P || !dS || !dqkv) return MFT_EINVAL;
    hipLaunchKernelGGL(feat_attention_bwd_rows_kernel, dim3(s.Ntok), dim3(FEAT_THREADS), 0, (hipStream_t)stream, d_o, qkv, P, m_att, s, dS,
                       dqkv);
    hipLaunchKernelGGL(feat_attention_bwd_cols_kernel, dim3(s.Ntok), dim3(FEAT_THREADS), 0, (hipStream_t)stream, d_o, qkv, P, m_att, dS, s,
                       dqkv);
    return mft_launch_status();
}

extern "C" int mft_feat_project_backward(const float* dqkv, const float* X, const float* dXres, int episodes, int n_way, int n_support,
                                         int n_query, int D, int train, const float* wq, const float* wk, const float* wv, float* dX,
                                         float* dW, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !dqkv || !X || !dXres || !wq || !wk || !wv || !dX || !dW)
        return MFT_EINVAL;
    const long long plane = (long long)s.Ntok * FEAT_D;
    FeatMm a = {};                                                  // dX[r, k] = dXres[r, k] + sum_z sum_n dqkv[z][r, n] Wz[n, k]
    for (int z = 0; z < 3; ++z) a.A[z] = dqkv + z * plane;
    a.B[0] = wq; a.B[1] = wk; a.B[2] = wv;
    a.sai = FEAT_D; a.sak = 1; a.sbj = 1; a.sbk = FEAT_D;
    a.M = s.Ntok; a.N = FEAT_D; a.K = FEAT_D; a.nseg = 3;
    a.add = dXres; a.C = dX; a.ldc = FEAT_D;
    int rc = launch_mm(a, 1, (hipStream_t)stream);
    if (rc != 0) return rc;
    FeatMm b = {};                                                  // dW[z][n, k] = sum_r dqkv[z][r, n] X[r, k], r in order
    for (int z = 0; z < 3; ++z) {
        b.A[z] = dqkv + z * plane;
        b.B[z] = X;
    }
    b.sai = 1; b.sak = FEAT_D; b.sbj = 1; b.sbk = FEAT_D;
    b.M = FEAT_D; b.N = FEAT_D; b.K = s.Ntok; b.nseg = 1;
    b.C = dW; b.ldc = FEAT_D; b.zc = (long long)FEAT_D * FEAT_D;
    return launch_mm(b, 3, (hipStream_t)stream);
}

extern "C" int mft_feat_dfeats(const float* ddirect, const float* dX, int episodes, int n_way, int n_support, int n_query, int D,
                               int train, float* dfeats, int ldd, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, train, s) || !al16(ddirect) || !al16(dX) || !rows_ok(dfeats, ldd))
        return MFT_EINVAL;
    hipLaunchKernelGGL(feat_dfeats_kernel, dim3(s.NP * s.T), dim3(128), 0, (hipStream_t)stream, ddirect, dX, s, train ? 1 : 0, dfeats, ldd);
    return mft_launch_status();
}

extern "C" int mft_feat_draw(int episodes, int n_way, int n_support, int n_query, int D, float p_att, float p_out,
                             unsigned long long seed, unsigned long long* index, const float* in_att, const float* in_out, float* m_att,
                             float* m_out, void* stream) {
    FeatShape s;
    if (!feat_shape(episodes, n_way, n_support, n_query, D, 1, s) || !index || !m_att || !m_out || (in_att == nullptr) != (in_out == nullptr) ||
        !(p_att >= 0.f && p_att < 1.f) || !(p_out >= 0.f && p_out < 1.f))
        return MFT_EINVAL;
    const long long n_att = (long long)s.NP * s.n_way + (long long)s.NP * s.T * s.T, n_out = (long long)s.Ntok * FEAT_D;
    hipLaunchKernelGGL(feat_draw_kernel, dim3(1), dim3(FEAT_DRAW_THREADS), 0, (hipStream_t)stream, n_att, n_out, p_att, p_out, seed, index,
                       in_att, in_out, m_att, m_out);
    return mft_launch_status();
}
