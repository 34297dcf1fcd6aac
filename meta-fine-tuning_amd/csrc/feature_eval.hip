// Episodic evaluation on frozen features: the top-1 count of every episode of a lockstep batch.
//
// MetaTemplate.correct takes the row maximum with torch.topk and reads the predictions back once per episode; the `test` driver
// scores E episodes with one head call and wants E integers.  One workgroup per episode: every thread walks rows
// tid, tid + 256, ... of its episode, scans the n_way scores of a row in column order, and keeps its own count; the 256 counts are
// added by a wave shuffle tree and a four-entry LDS pass.  Integer sums in a fixed tree: no atomics, the same bytes every run.
#include "mft_common.h"

namespace {

constexpr int TOP1_THREADS = 256;
constexpr int TOP1_MAX_WAY = 64;

// The lowest column attaining the row maximum over columns 0 .. n_way-1, with numpy's / torch's argmax order: a NaN is greater
// than every number, so the first NaN wins and nothing after it can replace it.  Columns >= n_way are never loaded.
__device__ __forceinline__ int row_argmax(const float* __restrict__ s, int n_way) {
    float best = s[0];
    int arg = 0;
    for (int c = 1; c < n_way; ++c) {
        const float v = s[c];
        if (best == best && (v > best || v != v)) {
            best = v;
            arg = c;
        }
    }
    return arg;
}

__global__ __launch_bounds__(TOP1_THREADS) void episode_top1_kernel(const float* __restrict__ scores, int ld, int n_way,
                                                                    int n_query, int* __restrict__ correct,
                                                                    int* __restrict__ pred) {
    __shared__ int part[TOP1_THREADS / MFT_WAVE];
    const int rows = n_way * n_query;                                  // <= 64 * n_query: the launcher bounds the product
    const long long row0 = (long long)blockIdx.x * rows;
    int hit = 0;
    for (int r = threadIdx.x; r < rows; r += TOP1_THREADS) {
        const int arg = row_argmax(scores + (row0 + r) * ld, n_way);
        if (pred) pred[row0 + r] = arg;
        hit += (arg == r / n_query) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hit += __shfl_xor(hit, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = hit;
    __syncthreads();
    if (threadIdx.x == 0) correct[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace

extern "C" int mft_episode_top1(const float* scores, int ld, int n_episodes, int n_way, int n_query, int* correct, int* pred,
                                void* stream) {
    if (n_way < 1 || n_way > TOP1_MAX_WAY || ld < n_way || n_query < 1 || n_episodes < 1) return MFT_EINVAL;
    if ((long long)n_way * n_query > 0x7fffffffLL) return MFT_EINVAL;  // rows of one episode are indexed with an int
    hipLaunchKernelGGL(episode_top1_kernel, dim3(n_episodes), dim3(TOP1_THREADS), 0, (hipStream_t)stream, scores, ld, n_way,
                       n_query, correct, pred);
    return mft_launch_status();
}
