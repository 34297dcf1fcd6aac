// Baseline++ head (backbone.distLinear: cosine classifier with a class-wise learnable norm), forward, backward and the whole
// test-time SGD adaptation of BaselineFinetune(loss_type='dist').set_forward_adaptation in one launch each.
//
//   n_r = ||x_r||, xh_r = x_r / (n_r + 1e-5);  w_c = g_c v_c / ||v_c||;  score[r,c] = s (xh_r . w_c), no bias.
//
// Layout: x rows of D floats (row stride ld), V [groups, C, D] and g [groups, C] contiguous, scores [rows, C] contiguous.
// wave64; a row's D <= 512 values sit in a wave as at most two float4 per lane (lanes past D / 4 hold zeros, so the arithmetic
// needs no tail test) and every dot product / norm is a wave butterfly sum.  Row and class norms are computed inside the launch
// that needs them.  The ~0.1-20 MFLOP of a call are latency-bound: the class loops fetch the next class's row of V before they
// reduce the current one.  Every sum runs in a fixed order (no atomics), so two launches on the same input are bit-identical.
#include "mft_common.h"

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_ROWS = 4;                  // rows of x per workgroup (forward, backward row role)
constexpr int DL_MAX_V4 = 2;                // D <= 512: at most two float4 per lane
constexpr int DL_MAX_C = 1024;
constexpr int DL_BWD_LDS_V4 = DL_WAVES * DL_ROWS * 128;      // 32 KiB: per-wave partial dxh rows of the backward row role
constexpr int DL_NORM_CHUNK = 1024;         // rows whose 1 / (n_r + eps) a class-role workgroup keeps in LDS at a time
constexpr float DL_EPS = 1e-5f;
static_assert(DL_ROWS == DL_WAVES, "the epilogues give row q of a workgroup to wave q");

typedef f32x4 DlRow[DL_MAX_V4];

__device__ __forceinline__ void dl_load(DlRow& r, const float* __restrict__ p, int d4, int lane) {
#pragma unroll
    for (int i = 0; i < DL_MAX_V4; ++i) {
        const int j = lane + 64 * i;
        r[i] = j < d4 ? *(const f32x4*)(p + 4 * j) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}

__device__ __forceinline__ void dl_store(float* __restrict__ p, const DlRow& r, int d4, int lane) {
#pragma unroll
    for (int i = 0; i < DL_MAX_V4; ++i) {
        const int j = lane + 64 * i;
        if (j < d4) *(f32x4*)(p + 4 * j) = r[i];
    }
}

// this lane's share of a . b (wave_sum of it is the dot product)
__device__ __forceinline__ float dl_dot(const DlRow& a, const DlRow& b) {
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < DL_MAX_V4; ++i) p += a[i].x * b[i].x + a[i].y * b[i].y + a[i].z * b[i].z + a[i].w * b[i].w;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (ceil(rows_per_group / 4), n_groups).  Each wave keeps the workgroup's four rows in registers and takes classes wave,
// wave + 4, ...: one read of v_c serves ||v_c|| and four dot products.  The scores of the four rows gather in LDS and leave
// as whole rows (row q by wave q), through the row softmax when asked.
__global__ __launch_bounds__(DL_THREADS) void dist_scores_kernel(const float* __restrict__ x, int ldx, int rpg,
                                                                 const float* __restrict__ V, const float* __restrict__ g, int C,
                                                                 int D, float s, float* __restrict__ scores, int softmax) {
    __shared__ float sc[DL_ROWS][DL_MAX_C];
    const int grp = blockIdx.y, r0 = blockIdx.x * DL_ROWS;
    const int nr = min(DL_ROWS, rpg - r0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d4 = D >> 2;
    const float* xg = x + ((long long)grp * rpg + r0) * ldx;
    const float* Vg = V + (long long)grp * C * D;
    const float* gg = g + (long long)grp * C;
    DlRow xr[DL_ROWS];
    float inv[DL_ROWS];
#pragma unroll
    for (int q = 0; q < DL_ROWS; ++q) {
        dl_load(xr[q], xg + (long long)min(q, nr - 1) * ldx, d4, lane);
        inv[q] = 1.f / (sqrtf(wave_sum(dl_dot(xr[q], xr[q]))) + DL_EPS);
    }
    DlRow vc, vn;
    int c = wave;
    if (c < C) dl_load(vc, Vg + (long long)c * D, d4, lane);
    for (; c < C; c += DL_WAVES) {
        if (c + DL_WAVES < C) dl_load(vn, Vg + (long long)(c + DL_WAVES) * D, d4, lane);
        const float coef = s * gg[c] / sqrtf(wave_sum(dl_dot(vc, vc)));
        float mine = 0.f;
#pragma unroll
        for (int q = 0; q < DL_ROWS; ++q) {
            const float d = wave_sum(dl_dot(xr[q], vc)) * inv[q] * coef;
            if (lane == q) mine = d;
        }
        if (lane < nr) sc[lane][c] = mine;
#pragma unroll
        for (int i = 0; i < DL_MAX_V4; ++i) vc[i] = vn[i];
    }
    __syncthreads();
    if (wave >= nr) return;
    const float* row = sc[wave];
    float* out = scores + ((long long)grp * rpg + r0 + wave) * C;
    if (!softmax) {
        for (int k = lane; k < C; k += 64) out[k] = row[k];
        return;
    }
    float mx = -3.4e38f;
    for (int k = lane; k < C; k += 64) mx = fmaxf(mx, row[k]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int k = lane; k < C; k += 64) se += expf(row[k] - mx);
    se = wave_sum(se);
    for (int k = lane; k < C; k += 64) out[k] = expf(row[k] - mx) / se;
}

// --------------------------------------------------------------------------------------------------------------- backward
// One launch, two roles.  With G = dL/dscore and A_c = sum_r G[r,c] xh_r:
//   row role   (workgroups [0, n_row_wgs), four rows each, only when dx is wanted):
//       dxh_r = s sum_c G[r,c] g_c v_c / ||v_c||;  dx_r = dxh_r / (n_r + eps) - x_r (dxh_r . x_r) / (n_r (n_r + eps)^2)
//       wave w sums its classes w, w + 4, ... for the four rows, the four partial rows meet in LDS and are added in wave order.
//   class role (the other workgroups, one class per wave):
//       P_c = sum_r G[r,c] u[r,c] = A_c . v_c / ||v_c||;  dg_c = s P_c;  dv_c = s g_c / ||v_c|| (A_c - P_c v_c / ||v_c||)
//       the rows are added in row order; 1 / (n_r + eps) of a chunk of rows is computed once per workgroup into LDS.
// Every element of dx, dV and dg is written exactly once: no zero fill, no atomics.
__global__ __launch_bounds__(DL_THREADS) void dist_backward_kernel(const float* __restrict__ x, int ldx, int R,
                                                                   const float* __restrict__ V, const float* __restrict__ g, int C,
                                                                   int D, float s, const float* __restrict__ G, int ldg,
                                                                   float* __restrict__ dx, int ldd, float* __restrict__ dV,
                                                                   float* __restrict__ dg, int n_row_wgs) {
    __shared__ f32x4 sm[DL_BWD_LDS_V4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d4 = D >> 2;
    if ((int)blockIdx.x < n_row_wgs) {
        const int r0 = blockIdx.x * DL_ROWS;
        const int nr = min(DL_ROWS, R - r0);
        DlRow acc[DL_ROWS];
#pragma unroll
        for (int q = 0; q < DL_ROWS; ++q)
#pragma unroll
            for (int i = 0; i < DL_MAX_V4; ++i) acc[q][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        DlRow vc, vn;
        int c = wave;
        if (c < C) dl_load(vc, V + (long long)c * D, d4, lane);
        for (; c < C; c += DL_WAVES) {
            if (c + DL_WAVES < C) dl_load(vn, V + (long long)(c + DL_WAVES) * D, d4, lane);
            const float w = g[c] / sqrtf(wave_sum(dl_dot(vc, vc)));
#pragma unroll
            for (int q = 0; q < DL_ROWS; ++q) {
                const float coef = q < nr ? G[(long long)(r0 + q) * ldg + c] * w : 0.f;
#pragma unroll
                for (int i = 0; i < DL_MAX_V4; ++i) acc[q][i] += coef * vc[i];
            }
#pragma unroll
            for (int i = 0; i < DL_MAX_V4; ++i) vc[i] = vn[i];
        }
#pragma unroll
        for (int q = 0; q < DL_ROWS; ++q)
#pragma unroll
            for (int i = 0; i < DL_MAX_V4; ++i) sm[(wave * DL_ROWS + q) * 128 + lane + 64 * i] = acc[q][i];
        __syncthreads();
        if (wave >= nr) return;
        DlRow dxh, xr;
#pragma unroll
        for (int i = 0; i < DL_MAX_V4; ++i) {
            f32x4 t = sm[wave * 128 + lane + 64 * i];
            for (int w = 1; w < DL_WAVES; ++w) t += sm[(w * DL_ROWS + wave) * 128 + lane + 64 * i];
            dxh[i] = s * t;
        }
        dl_load(xr, x + (long long)(r0 + wave) * ldx, d4, lane);
        const float n = sqrtf(wave_sum(dl_dot(xr, xr)));
        const float ie = 1.f / (n + DL_EPS);
        const float p = wave_sum(dl_dot(dxh, xr));
        const float k2 = n > 0.f ? p * ie * ie / n : 0.f;
#pragma unroll
        for (int i = 0; i < DL_MAX_V4; ++i) dxh[i] = dxh[i] * ie - xr[i] * k2;
        dl_store(dx + (long long)(r0 + wave) * ldd, dxh, d4, lane);
        return;
    }
    float* invn = (float*)sm;
    const int c = ((int)blockIdx.x - n_row_wgs) * DL_WAVES + wave;
    const bool live = c < C;
    DlRow A;
#pragma unroll
    for (int i = 0; i < DL_MAX_V4; ++i) A[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int rb = 0; rb < R; rb += DL_NORM_CHUNK) {
        const int nrb = min(DL_NORM_CHUNK, R - rb);
        __syncthreads();
        for (int r = wave; r < nrb; r += DL_WAVES) {
            DlRow xr;
            dl_load(xr, x + (long long)(rb + r) * ldx, d4, lane);
            const float n = sqrtf(wave_sum(dl_dot(xr, xr)));
            if (lane == 0) invn[r] = 1.f / (n + DL_EPS);
        }
        __syncthreads();
        if (!live) continue;
#pragma unroll 4
        for (int r = 0; r < nrb; ++r) {
            DlRow xr;
            dl_load(xr, x + (long long)(rb + r) * ldx, d4, lane);
            const float coef = G[(long long)(rb + r) * ldg + c] * invn[r];
#pragma unroll
            for (int i = 0; i < DL_MAX_V4; ++i) A[i] += coef * xr[i];
        }
    }
    if (!live) return;
    DlRow vc;
    dl_load(vc, V + (long long)c * D, d4, lane);
    const float nv = sqrtf(wave_sum(dl_dot(vc, vc)));
    const float P = wave_sum(dl_dot(A, vc)) / nv;
    const float k1 = s * g[c] / nv, k2 = P / nv;
#pragma unroll
    for (int i = 0; i < DL_MAX_V4; ++i) A[i] = k1 * (A[i] - k2 * vc[i]);
    dl_store(dV + (long long)c * D, A, d4, lane);
    if (lane == 0) dg[c] = s * P;
}

// ------------------------------------------------------------------------------------------- head adaptation, the whole run
// BaselineFinetune(loss_type='dist').set_forward_adaptation (baselinefinetune.py:17-58): a fresh distLinear(D, n_way) trained on
// the frozen support features with torch.optim.SGD(lr, momentum, dampening, weight_decay) on both g and v, n_steps mini-batches
// of <= bs rows named by the index table (-1 = empty slot), loss = mean cross entropy of the mini-batch.  One workgroup per group
// keeps V, its momentum buffer, g and 1 / (n_r + eps) of every support row in LDS and runs all steps in one launch.
// ZLDS: the support rows sit in LDS as well; otherwise a step reads its <= bs rows (twice) from HBM / L2.
// A step:  (A) wave tasks: ||v_c|| for every class, x_r . v_c for every (row, class) of the mini-batch;
//          (B) one thread per row: u = dot / ||v_c||, logits s g_c u, softmax, G = (p - onehot) / k; one thread per class:
//              s g_c / ||v_c|| (the V update must not read g while the g update writes it);
//          (C) one thread per float4 of V: dv as in the backward kernel with P_c = sum_r G[r,c] u[r,c], then the SGD update;
//              n_way threads update g; bs threads put the next step's rows and labels (fetched at the top of the step) in LDS.
template <bool ZLDS>
__global__ __launch_bounds__(DL_THREADS) void dist_head_sgd_kernel(const float* __restrict__ z, const int* __restrict__ y,
                                                                   const int* __restrict__ idx, int S, int D, int n_way, int T,
                                                                   int bs, float* __restrict__ V, float* __restrict__ g, float s,
                                                                   float lr, float mom, float damp, float wd) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    const int grp = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d4 = D >> 2;
    float* zl = dsm;                              // [S][D] (ZLDS only)
    float* Vs = zl + (ZLDS ? S * D : 0);          // [n_way][D]
    float* Bv = Vs + n_way * D;                   // momentum buffer of V
    float* dl = Bv + n_way * D;                   // [16][16] x_r . v_c / (n_r + eps), then u
    float* sl = dl + 256;                         // [16][16] logits, then G
    float* nvl = sl + 256;                        // [16] ||v_c||
    float* cf = nvl + 16;                         // [16] s g_c / ||v_c||
    float* gs = cf + 16;                          // [16] g
    float* gb = gs + 16;                          // [16] momentum buffer of g
    int* rid = (int*)(gb + 16);                   // [2][16] support rows of this / the next mini-batch
    int* ryl = rid + 32;                          // [2][16] their labels
    float* inv = (float*)(ryl + 32);              // [S] 1 / (n_r + eps)
    const float* zg = z + (long long)grp * S * D;
    const int* yg = y + (long long)grp * S;
    const int* ig = idx + (long long)grp * T * bs;
    if (ZLDS)
        for (int i = tid; i < S * d4; i += DL_THREADS) ((f32x4*)zl)[i] = ((const f32x4*)zg)[i];
    for (int i = tid; i < n_way * d4; i += DL_THREADS) {
        ((f32x4*)Vs)[i] = ((const f32x4*)(V + (long long)grp * n_way * D))[i];
        ((f32x4*)Bv)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    for (int r = wave; r < S; r += DL_WAVES) {
        DlRow xr;
        dl_load(xr, zg + (long long)r * D, d4, lane);
        const float n = sqrtf(wave_sum(dl_dot(xr, xr)));
        if (lane == 0) inv[r] = 1.f / (n + DL_EPS);
    }
    if (tid < n_way) { gs[tid] = g[(long long)grp * n_way + tid]; gb[tid] = 0.f; }
    if (tid < bs) {
        const int id = ig[tid];
        rid[tid] = id < 0 ? -1 : min(id, S - 1);
        ryl[tid] = id < 0 ? 0 : yg[min(id, S - 1)];
    }
    __syncthreads();
    const float* zs = ZLDS ? (const float*)zl : zg;
    for (int t = 0; t < T; ++t) {
        const int* rd = rid + (t & 1) * 16;
        const int* ry = ryl + (t & 1) * 16;
        int nid = -1, ny = 0;                      // the next mini-batch: fetched now, stored after phase C
        const bool fetch = tid >= 128 && tid < 128 + bs && t + 1 < T;
        if (fetch) {
            nid = ig[(long long)(t + 1) * bs + tid - 128];
            nid = nid < 0 ? -1 : min(nid, S - 1);
            ny = nid < 0 ? 0 : yg[nid];
        }
        int k = 0;
        while (k < bs && rd[k] >= 0) ++k;         // ragged tail: -1 padded
        // (A)
        for (int task = wave; task < n_way + k * n_way; task += DL_WAVES) {
            DlRow vc;
            if (task < n_way) {
                dl_load(vc, Vs + task * D, d4, lane);
                const float nv = sqrtf(wave_sum(dl_dot(vc, vc)));
                if (lane == 0) nvl[task] = nv;
            } else {
                const int pr = task - n_way, r = pr / n_way, c = pr - r * n_way;
                const int row = rd[r];
                DlRow xr;
                dl_load(xr, zs + (long long)row * D, d4, lane);
                dl_load(vc, Vs + c * D, d4, lane);
                const float d = wave_sum(dl_dot(xr, vc));
                if (lane == 0) dl[r * 16 + c] = d * inv[row];
            }
        }
        __syncthreads();
        // (B)
        if (tid < k) {
            const int r = tid;
            float mx = -3.4e38f;
            for (int c = 0; c < n_way; ++c) {
                const float u = dl[r * 16 + c] / nvl[c];
                const float lg = s * gs[c] * u;
                dl[r * 16 + c] = u;
                sl[r * 16 + c] = lg;
                mx = fmaxf(mx, lg);
            }
            float se = 0.f;
            for (int c = 0; c < n_way; ++c) se += expf(sl[r * 16 + c] - mx);
            const float lse = mx + logf(se);
            const int yy = ry[r];
            const float ik = 1.f / (float)k;
            for (int c = 0; c < n_way; ++c) sl[r * 16 + c] = (expf(sl[r * 16 + c] - lse) - (c == yy ? 1.f : 0.f)) * ik;
        } else if (tid >= 64 && tid < 64 + n_way) {
            const int c = tid - 64;
            cf[c] = s * gs[c] / nvl[c];
        }
        __syncthreads();
        // (C)
        for (int i = tid; i < n_way * d4; i += DL_THREADS) {
            const int c = i / d4, j = i - c * d4;
            f32x4 A = {0.f, 0.f, 0.f, 0.f};
            float P = 0.f;
            for (int r = 0; r < k; ++r) {
                const float grc = sl[r * 16 + c];
                const int row = rd[r];
                P += grc * dl[r * 16 + c];
                A += (grc * inv[row]) * *(const f32x4*)(zs + (long long)row * D + 4 * j);
            }
            const f32x4 v = ((f32x4*)Vs)[i];
            const f32x4 gr = cf[c] * (A - (P / nvl[c]) * v) + wd * v;
            const f32x4 bu = t == 0 ? gr : mom * ((f32x4*)Bv)[i] + (1.f - damp) * gr;
            ((f32x4*)Bv)[i] = bu;
            ((f32x4*)Vs)[i] = v - lr * bu;
        }
        if (tid < n_way) {
            float P = 0.f;
            for (int r = 0; r < k; ++r) P += sl[r * 16 + tid] * dl[r * 16 + tid];
            const float w = gs[tid];
            const float gr = s * P + wd * w;
            const float bu = t == 0 ? gr : mom * gb[tid] + (1.f - damp) * gr;
            gb[tid] = bu;
            gs[tid] = w - lr * bu;
        }
        if (fetch) {
            rid[((t + 1) & 1) * 16 + tid - 128] = nid;
            ryl[((t + 1) & 1) * 16 + tid - 128] = ny;
        }
        __syncthreads();
    }
    for (int i = tid; i < n_way * d4; i += DL_THREADS) ((f32x4*)(V + (long long)grp * n_way * D))[i] = ((const f32x4*)Vs)[i];
    if (tid < n_way) g[(long long)grp * n_way + tid] = gs[tid];
}

// ------------------------------------------------------------------------------- test-time head step (FinetuneEngine "dist")
// The cosine counterpart of linear_head_step_kernel (csrc/loss_optim.hip): one inner step of finetune_linear with a
// distLinear(D, n_way) head for all episodes of the batch, one workgroup per episode (group).  feat -> scores -> mean cross
// entropy -> dfeat (pre-update V, g) -> Adam with L2 weight decay on V and g.  k <= 16 rows, n_way <= 16.
//   (A) wave tasks: ||v_c|| for class wave, wave + 4, ...; for row wave, wave + 4, ...: n_r and x_r . v_c for every class;
//   (B) one thread per row: u, logits s g_c u, softmax, G = (p - onehot) / k, the row's loss; one thread per class: s g_c / ||v_c||;
//   (C) one wave per row: dxh_r = sum_c G[r,c] (s g_c / ||v_c||) v_c in class order, dx_r as in the backward kernel; thread 0: loss;
//   (D) behind a barrier (every read of V and g for dfeat is done): one thread per float4 of V: dv as in the run kernel with
//       P_c = sum_r G[r,c] u[r,c], weight decay, Adam; n_way threads do the same for g (they read g only through phase B's LDS copy).
constexpr int DH_MAX = 16;

__global__ __launch_bounds__(DL_THREADS) void dist_head_step_kernel(
    const float* __restrict__ feat, int ldf, const int* __restrict__ labels, int k, int n_way, int D, float s,
    float* __restrict__ V, float* __restrict__ g, float* __restrict__ mV, float* __restrict__ vV, float* __restrict__ mg,
    float* __restrict__ vg, float* __restrict__ dfeat, int lddf, float* __restrict__ loss, float step_size, float inv_sqrt_bc2,
    float b1, float b2, float c1, float c2, float eps, float wd) {
    __shared__ float sU[DH_MAX][DH_MAX];       // x_r . v_c, then u[r,c]
    __shared__ float sG[DH_MAX][DH_MAX];       // G[r,c]
    __shared__ float s_n[DH_MAX];              // n_r
    __shared__ float s_inv[DH_MAX];            // 1 / (n_r + eps_n)
    __shared__ float s_inv_nv[DH_MAX];         // 1 / ||v_c||
    __shared__ float s_cf[DH_MAX];             // s g_c / ||v_c||
    __shared__ float s_g[DH_MAX];              // g_c before the update
    __shared__ float s_loss[DH_MAX];
    const int grp = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d4 = D >> 2;
    const float* F = feat + (long long)grp * k * ldf;
    float* Vg = V + (long long)grp * n_way * D;
    float* gg = g + (long long)grp * n_way;
    // (A)
    for (int c = wave; c < n_way; c += DL_WAVES) {
        DlRow vc;
        dl_load(vc, Vg + (long long)c * D, d4, lane);
        const float nv = sqrtf(wave_sum(dl_dot(vc, vc)));
        if (lane == 0) s_inv_nv[c] = 1.f / nv;
    }
    for (int r = wave; r < k; r += DL_WAVES) {
        DlRow xr, vc, vn;
        dl_load(xr, F + (long long)r * ldf, d4, lane);
        dl_load(vc, Vg, d4, lane);
        const float n = sqrtf(wave_sum(dl_dot(xr, xr)));
        if (lane == 0) { s_n[r] = n; s_inv[r] = 1.f / (n + DL_EPS); }
        for (int c = 0; c < n_way; ++c) {
            if (c + 1 < n_way) dl_load(vn, Vg + (long long)(c + 1) * D, d4, lane);
            const float d = wave_sum(dl_dot(xr, vc));
            if (lane == 0) sU[r][c] = d;
#pragma unroll
            for (int i = 0; i < DL_MAX_V4; ++i) vc[i] = vn[i];
        }
    }
    __syncthreads();
    // (B)
    if (tid < k) {
        const int r = tid;
        const int y = labels[(long long)grp * k + r];
        const float ir = s_inv[r];
        float mx = -3.4e38f;
        for (int c = 0; c < n_way; ++c) {
            const float u = sU[r][c] * ir * s_inv_nv[c];
            const float lg = s * gg[c] * u;
            sU[r][c] = u;
            sG[r][c] = lg;
            mx = fmaxf(mx, lg);
        }
        float se = 0.f;
        for (int c = 0; c < n_way; ++c) se += expf(sG[r][c] - mx);
        const float lse = mx + logf(se);
        const float ik = 1.f / (float)k;
        float ly = 0.f;
        for (int c = 0; c < n_way; ++c) {
            const float lg = sG[r][c];
            if (c == y) ly = lg;
            sG[r][c] = (expf(lg - lse) - (c == y ? 1.f : 0.f)) * ik;
        }
        s_loss[r] = lse - ly;
    } else if (tid >= 64 && tid < 64 + n_way) {
        const int c = tid - 64;
        const float gc = gg[c];
        s_g[c] = gc;
        s_cf[c] = s * gc * s_inv_nv[c];
    }
    __syncthreads();
    // (C)
    if (tid == 0 && loss != nullptr) {
        float t = 0.f;
        for (int r = 0; r < k; ++r) t += s_loss[r];
        loss[grp] = t / (float)k;
    }
    for (int r = wave; r < k; r += DL_WAVES) {
        DlRow xr, vc, vn, dxh;
        dl_load(xr, F + (long long)r * ldf, d4, lane);
        dl_load(vc, Vg, d4, lane);
#pragma unroll
        for (int i = 0; i < DL_MAX_V4; ++i) dxh[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < n_way; ++c) {
            if (c + 1 < n_way) dl_load(vn, Vg + (long long)(c + 1) * D, d4, lane);
            const float coef = sG[r][c] * s_cf[c];
#pragma unroll
            for (int i = 0; i < DL_MAX_V4; ++i) {
                dxh[i] += coef * vc[i];
                vc[i] = vn[i];
            }
        }
        const float n = s_n[r], ie = s_inv[r];
        const float p = wave_sum(dl_dot(dxh, xr));
        const float k2 = n > 0.f ? p * ie * ie / n : 0.f;
#pragma unroll
        for (int i = 0; i < DL_MAX_V4; ++i) dxh[i] = dxh[i] * ie - xr[i] * k2;
        dl_store(dfeat + ((long long)grp * k + r) * lddf, dxh, d4, lane);
    }
    __syncthreads();
    // (D)
    f32x4* mVg = (f32x4*)(mV + (long long)grp * n_way * D);
    f32x4* vVg = (f32x4*)(vV + (long long)grp * n_way * D);
    for (int i = tid; i < n_way * d4; i += DL_THREADS) {
        const int c = i / d4, j = i - c * d4;
        f32x4 A = {0.f, 0.f, 0.f, 0.f};
        float P = 0.f;
        for (int r = 0; r < k; ++r) {
            const float grc = sG[r][c];
            P += grc * sU[r][c];
            A += (grc * s_inv[r]) * *(const f32x4*)(F + (long long)r * ldf + 4 * j);
        }
        f32x4 w = ((f32x4*)Vg)[i], m = mVg[i], v = vVg[i];
        const f32x4 gr = s_cf[c] * (A - (P * s_inv_nv[c]) * w) + wd * w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[e] = b1 * m[e] + c1 * gr[e];
            v[e] = b2 * v[e] + c2 * gr[e] * gr[e];
            w[e] = w[e] - step_size * (m[e] / (sqrtf(v[e]) * inv_sqrt_bc2 + eps));
        }
        mVg[i] = m;
        vVg[i] = v;
        ((f32x4*)Vg)[i] = w;
    }
    if (tid < n_way) {
        const int c = tid;
        float P = 0.f;
        for (int r = 0; r < k; ++r) P += sG[r][c] * sU[r][c];
        const float w = s_g[c];
        const float gr = s * P + wd * w;
        const long long i = (long long)grp * n_way + c;
        const float m = b1 * mg[i] + c1 * gr;
        const float v = b2 * vg[i] + c2 * gr * gr;
        mg[i] = m;
        vg[i] = v;
        gg[c] = w - step_size * (m / (sqrtf(v) * inv_sqrt_bc2 + eps));
    }
}

// torch.optim.Adam forms 1 - beta and the bias corrections in double from the decimal beta it was given (0.999 -> 0.001); a beta
// that arrives here as a float is 1.3e-5 of 1 - beta away from that (1.f - 0.999f = 0.00099998713), which is the whole error of v
// after a first step from zero moments.  -> the beta rounded to 7 decimals: the decimal itself, or within a float ulp of any other.
double dl_beta_decimal(float beta) { return nearbyint((double)beta * 1e7) / 1e7; }

bool dl_dims_ok(int C, int D) { return C >= 1 && C <= DL_MAX_C && D >= 4 && D <= 512 && (D & 3) == 0; }
bool dl_rows_ok(const void* p, int ld, int D) { return p != nullptr && ld >= D && (ld & 3) == 0 && ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mft_dist_linear_forward(const float* x, int ldx, int n_groups, int rows_per_group, const float* V, const float* g,
                                       int C, int D, float s, float* scores, int softmax, void* stream) {
    if (!dl_dims_ok(C, D) || !dl_rows_ok(x, ldx, D) || !dl_rows_ok(V, D, D) || g == nullptr || scores == nullptr) return MFT_EINVAL;
    if (n_groups < 1 || n_groups > 65535 || rows_per_group < 1) return MFT_EINVAL;
    hipLaunchKernelGGL(dist_scores_kernel, dim3(cdiv(rows_per_group, DL_ROWS), n_groups), dim3(DL_THREADS), 0, (hipStream_t)stream,
                       x, ldx, rows_per_group, V, g, C, D, s, scores, softmax ? 1 : 0);
    return mft_launch_status();
}

extern "C" int mft_dist_linear_backward(const float* x, int ldx, int rows, const float* V, const float* g, int C, int D, float s,
                                        const float* dscores, int ldg, float* dx, int ldd, float* dV, float* dg, void* stream) {
    if (!dl_dims_ok(C, D) || !dl_rows_ok(x, ldx, D) || !dl_rows_ok(V, D, D) || !dl_rows_ok(dV, D, D)) return MFT_EINVAL;
    if (g == nullptr || dg == nullptr || dscores == nullptr || ldg < C || rows < 1) return MFT_EINVAL;
    if (dx != nullptr && !dl_rows_ok(dx, ldd, D)) return MFT_EINVAL;
    const int n_row_wgs = dx != nullptr ? cdiv(rows, DL_ROWS) : 0;
    hipLaunchKernelGGL(dist_backward_kernel, dim3(n_row_wgs + cdiv(C, DL_WAVES)), dim3(DL_THREADS), 0, (hipStream_t)stream, x, ldx,
                       rows, V, g, C, D, s, dscores, ldg, dx, ldd, dV, dg, n_row_wgs);
    return mft_launch_status();
}

extern "C" int mft_dist_head_sgd_run(const float* z_support, const int* y_support, const int* idx_table, int n_groups,
                                     int n_support_rows, int D, int n_way, int n_steps, int batch_size, float* V, float* g, float s,
                                     float lr, float momentum, float dampening, float weight_decay, void* stream) {
    if (n_way < 1 || n_way > 16 || batch_size < 1 || batch_size > 16 || n_steps < 1 || n_groups < 1 || n_support_rows < 1)
        return MFT_EINVAL;
    if (!dl_dims_ok(n_way, D) || !dl_rows_ok(z_support, D, D) || !dl_rows_ok(V, D, D)) return MFT_EINVAL;
    if (g == nullptr || y_support == nullptr || idx_table == nullptr) return MFT_EINVAL;
    const size_t lds_cap = 150 * 1024;
    const size_t head = (2 * (size_t)n_way * D + 2 * 256 + 4 * 16 + 2 * 32 + (((size_t)n_support_rows + 3) & ~(size_t)3)) * sizeof(float);
    const size_t lds_z = (size_t)n_support_rows * D * sizeof(float) + head;
    if (head > lds_cap) return MFT_EINVAL;
    static MftPerDeviceOnce attr_once;
    if (attr_once.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)dist_head_sgd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds_cap);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)dist_head_sgd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_cap);
        if (e != hipSuccess) return (int)e;
        attr_once.mark();
    }
    if (lds_z <= lds_cap)
        hipLaunchKernelGGL((dist_head_sgd_kernel<true>), dim3(n_groups), dim3(DL_THREADS), lds_z, (hipStream_t)stream, z_support,
                           y_support, idx_table, n_support_rows, D, n_way, n_steps, batch_size, V, g, s, lr, momentum, dampening,
                           weight_decay);
    else
        hipLaunchKernelGGL((dist_head_sgd_kernel<false>), dim3(n_groups), dim3(DL_THREADS), head, (hipStream_t)stream, z_support,
                           y_support, idx_table, n_support_rows, D, n_way, n_steps, batch_size, V, g, s, lr, momentum, dampening,
                           weight_decay);
    return mft_launch_status();
}

extern "C" int mft_dist_head_step(const float* feat, int ldf, const int* labels, int rows_per_group, int n_groups, int n_way, int D,
                                  float s, float* V, float* g, float* mV, float* vV, float* mg, float* vg, float* dfeat, int lddf,
                                  float* loss, int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  void* stream) {
    if (step < 1 || n_groups < 1 || rows_per_group < 1 || rows_per_group > DH_MAX || n_way < 1 || n_way > DH_MAX) return MFT_EINVAL;
    if (!dl_dims_ok(n_way, D) || !dl_rows_ok(feat, ldf, D) || !dl_rows_ok(dfeat, lddf, D)) return MFT_EINVAL;
    if (!dl_rows_ok(V, D, D) || !dl_rows_ok(mV, D, D) || !dl_rows_ok(vV, D, D)) return MFT_EINVAL;
    if (labels == nullptr || g == nullptr || mg == nullptr || vg == nullptr) return MFT_EINVAL;
    const double b1d = dl_beta_decimal(beta1), b2d = dl_beta_decimal(beta2);
    const double bc1 = 1.0 - pow(b1d, (double)step);
    const double bc2 = 1.0 - pow(b2d, (double)step);
    hipLaunchKernelGGL(dist_head_step_kernel, dim3(n_groups), dim3(DL_THREADS), 0, (hipStream_t)stream, feat, ldf, labels,
                       rows_per_group, n_way, D, s, V, g, mV, vV, mg, vg, dfeat, lddf, loss, (float)((double)lr / bc1),
                       (float)(1.0 / sqrt(bc2)), beta1, beta2, (float)(1.0 - b1d), (float)(1.0 - b2d), eps, weight_decay);
    return mft_launch_status();
}
