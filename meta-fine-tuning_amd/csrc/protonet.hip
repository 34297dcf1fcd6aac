// ProtoNet head (methods/protonet.py: set_forward + euclidean_dist) forward and backward, every episode of a step in one launch.
//
// Layout: feats [episodes, n_way, n_support + n_query, D] with row stride ld (the rows the meta-training forward and the engine's
// final pass write); scores [episodes * n_way * n_query, n_way], query rows class-major inside an episode (c * n_query + q).
//
// One 256-thread workgroup per episode.  The prototypes live in LDS in chunks of PROTO_LDS_FLOATS / D classes (16 at D = 512), so
// the static 32 KiB of LDS covers every n_way <= 64 without a dynamic-LDS attribute.  A query row belongs to one wave (row % 4)
// in every chunk; each lane holds D / 64 of its features as float4 and the distance is a wave butterfly sum.  All sums run in a
// fixed order (no atomics), so two launches on the same input are bit-identical.
#include "mft_common.h"

namespace {

constexpr int PROTO_THREADS = 256;
constexpr int PROTO_LDS_FLOATS = 8192;      // 32 KiB
constexpr int PROTO_MAX_V4 = 2;             // D <= 512: at most two float4 per lane

struct ProtoShape {
    int n_way, ns, nq, D, ld;
};

// prototypes of classes [c0, c0 + cb) of one episode into LDS: sum of the support rows in row order, then / n_support
__device__ __forceinline__ void load_protos(f32x4* __restrict__ sp, const float* __restrict__ ep, const ProtoShape s, int c0,
                                            int cb) {
    const int d4 = s.D >> 2;
    const int per = s.ns + s.nq;
    for (int i = threadIdx.x; i < cb * d4; i += PROTO_THREADS) {
        const int c = i / d4, j = i - c * d4;
        const float* src = ep + (long long)(c0 + c) * per * s.ld + 4 * j;
        f32x4 acc = *(const f32x4*)src;
        for (int r = 1; r < s.ns; ++r) acc += *(const f32x4*)(src + (long long)r * s.ld);
        sp[c * d4 + j] = acc / (f32x4){(float)s.ns, (float)s.ns, (float)s.ns, (float)s.ns};
    }
}

__global__ __launch_bounds__(PROTO_THREADS) void proto_scores_kernel(const float* __restrict__ feats, ProtoShape s,
                                                                     float* __restrict__ scores, int softmax) {
    __shared__ f32x4 sp[PROTO_LDS_FLOATS / 4];
    const int e = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = s.ns + s.nq, d4 = s.D >> 2;
    const int cmax = PROTO_LDS_FLOATS / s.D;
    const int qrows = s.n_way * s.nq;
    const float* ep = feats + (long long)e * s.n_way * per * s.ld;
    float* out = scores + (long long)e * qrows * s.n_way;
    for (int c0 = 0; c0 < s.n_way; c0 += cmax) {
        const int cb = min(cmax, s.n_way - c0);
        __syncthreads();
        load_protos(sp, ep, s, c0, cb);
        __syncthreads();
        for (int r = wave; r < qrows; r += PROTO_THREADS / 64) {
            const int c = r / s.nq, q = r - c * s.nq;
            const float* x = ep + (long long)(c * per + s.ns + q) * s.ld;
            f32x4 xv[PROTO_MAX_V4];
#pragma unroll
            for (int i = 0; i < PROTO_MAX_V4; ++i) {
                const int j = lane + 64 * i;
                xv[i] = j < d4 ? *(const f32x4*)(x + 4 * j) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            for (int k = 0; k < cb; ++k) {
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < PROTO_MAX_V4; ++i) {
                    const int j = lane + 64 * i;
                    if (j < d4) {
                        const f32x4 t = xv[i] - sp[k * d4 + j];
                        part += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
                    }
                }
                part = wave_sum(part);
                if (lane == 0) out[(long long)r * s.n_way + c0 + k] = -part;
            }
        }
    }
    if (!softmax) return;
    __syncthreads();        // every score of the episode is written (workgroup-scope visibility of the global stores)
    for (int r = wave; r < qrows; r += PROTO_THREADS / 64) {
        float* row = out + (long long)r * s.n_way;
        const float v = lane < s.n_way ? row[lane] : -3.4e38f;
        const float mx = wave_max(v);
        const float ex = lane < s.n_way ? expf(v - mx) : 0.f;
        const float se = wave_sum(ex);
        if (lane < s.n_way) row[lane] = ex / se;
    }
}

// dq  = -2 (sum_c g_qc q - sum_c g_qc p_c)  = sum_c -2 g_qc (q - p_c), accumulated over the classes in order
// dsupport(c) = (sum_q 2 g_qc (q - p_c)) / n_support, the same row for every support image of class c
__global__ __launch_bounds__(PROTO_THREADS) void proto_backward_kernel(const float* __restrict__ feats, ProtoShape s,
                                                                       const float* __restrict__ dscores, int ldg,
                                                                       float* __restrict__ dfeats, int ldd) {
    __shared__ f32x4 sp[PROTO_LDS_FLOATS / 4];
    const int e = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = s.ns + s.nq, d4 = s.D >> 2;
    const int cmax = PROTO_LDS_FLOATS / s.D;
    const int qrows = s.n_way * s.nq;
    const float* ep = feats + (long long)e * s.n_way * per * s.ld;
    float* dep = dfeats + (long long)e * s.n_way * per * ldd;
    const float* g = dscores + (long long)e * qrows * ldg;
    const float two_ns = 2.f / (float)s.ns;
    for (int c0 = 0; c0 < s.n_way; c0 += cmax) {
        const int cb = min(cmax, s.n_way - c0);
        __syncthreads();
        load_protos(sp, ep, s, c0, cb);
        __syncthreads();
        // query rows: one wave per row, the chunk's classes added to what the earlier chunks left (same lane, same address)
        for (int r = wave; r < qrows; r += PROTO_THREADS / 64) {
            const int c = r / s.nq, q = r - c * s.nq;
            const long long row = (long long)(c * per + s.ns + q);
            const float* x = ep + row * s.ld;
            float* dx = dep + row * ldd;
            const float* gr = g + (long long)r * ldg;
#pragma unroll
            for (int i = 0; i < PROTO_MAX_V4; ++i) {
                const int j = lane + 64 * i;
                if (j >= d4) continue;
                const f32x4 xv = *(const f32x4*)(x + 4 * j);
                f32x4 acc = c0 == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(dx + 4 * j);
                for (int k = 0; k < cb; ++k) {
                    const float w = -2.f * gr[c0 + k];
                    acc += w * (xv - sp[k * d4 + j]);
                }
                *(f32x4*)(dx + 4 * j) = acc;
            }
        }
        // support rows of the chunk's classes: one (class, float4 column) per thread, the query rows summed in row order
        for (int i = threadIdx.x; i < cb * d4; i += PROTO_THREADS) {
            const int k = i / d4, j = i - k * d4;
            const int c = c0 + k;
            const f32x4 p = sp[k * d4 + j];
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < qrows; ++r) {
                const int cq = r / s.nq, q = r - cq * s.nq;
                const f32x4 xv = *(const f32x4*)(ep + (long long)(cq * per + s.ns + q) * s.ld + 4 * j);
                acc += g[(long long)r * ldg + c] * (xv - p);
            }
            acc *= two_ns;
            for (int sr = 0; sr < s.ns; ++sr) *(f32x4*)(dep + (long long)(c * per + sr) * ldd + 4 * j) = acc;
        }
    }
}

bool proto_shape_ok(const void* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D) {
    if (feats == nullptr || episodes < 1 || n_way < 1 || n_way > 64 || n_support < 1 || n_query < 1) return false;
    if (D < 4 || D > 512 || (D & 3) != 0 || ld < D || (ld & 3) != 0) return false;
    return ((uintptr_t)feats & 15) == 0;
}

}  // namespace

extern "C" int mft_proto_scores(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                float* scores, int softmax, void* stream) {
    if (!proto_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || scores == nullptr) return MFT_EINVAL;
    const ProtoShape s = {n_way, n_support, n_query, D, ld};
    hipLaunchKernelGGL(proto_scores_kernel, dim3(episodes), dim3(PROTO_THREADS), 0, (hipStream_t)stream, feats, s, scores,
                       softmax ? 1 : 0);
    return mft_launch_status();
}

extern "C" int mft_proto_backward(const float* feats, int ld, int episodes, int n_way, int n_support, int n_query, int D,
                                  const float* dscores, int ldg, float* dfeats, int ldd, void* stream) {
    if (!proto_shape_ok(feats, ld, episodes, n_way, n_support, n_query, D) || dscores == nullptr || dfeats == nullptr)
        return MFT_EINVAL;
    if (ldg < n_way || ldd < D || (ldd & 3) != 0 || ((uintptr_t)dfeats & 15) != 0) return MFT_EINVAL;
    const ProtoShape s = {n_way, n_support, n_query, D, ld};
    hipLaunchKernelGGL(proto_backward_kernel, dim3(episodes), dim3(PROTO_THREADS), 0, (hipStream_t)stream, feats, s, dscores, ldg,
                       dfeats, ldd);
    return mft_launch_status();
}
