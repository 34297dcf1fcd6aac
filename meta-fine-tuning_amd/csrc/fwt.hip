// Feature-wise transformation layers of ResNet10_FW (backbone.py:313-350 of the reference: FeatureWiseTransformation2d_fw), all
// seven layers of the backbone and all lockstep groups in one launch each way.
//
// Train mode:  y = gm * BatchNorm(x) + bt,  gm = 1 + n_g * softplus(gamma),  bt = n_b * softplus(beta),  n_g, n_b ~ N(0, 1) one
// value per channel.  Per-channel noise makes the layer a BatchNorm with the affine (w', b') = (gm * w, gm * b + bt):
//   fwt_draw_fold_kernel   draws the normals, writes w', b' [groups, C] for the BatchNorm launchers (gb_group_stride = C), keeps gm
//                          and the noise [groups, 2, ld] for the backward, and advances the draw index in device memory;
//   fwt_unfold_kernel      turns the BatchNorm backward's per-group gradients of (w', b') into those of w, b, gamma, beta.
//
// Generator: Philox4x32-10, counter = (column in the noise layout, group, draw index low, draw index high), key = the 64-bit seed.
// Words 0 and 1 of the output become two uniforms in (0, 1) and one Box-Muller pair, evaluated in double and rounded once.
// The draw index is read by every thread, then -- behind a barrier -- advanced by thread 0: the launch is ONE workgroup (at most
// 3,712 values per group), so nothing waits on another workgroup and a replayed hipGraph draws fresh noise every step.
#include "philox.h"

namespace {

constexpr int FWT_MAX_LAYERS = 8;
constexpr int FWT_MAX_C = 512;
constexpr int FWT_FOLD_THREADS = 1024;
constexpr int FWT_UNFOLD_THREADS = 256;

struct FwtFoldArgs {
    MftFwtJob job[FWT_MAX_LAYERS];
    int n, groups, ld;
    unsigned long long seed;
    unsigned long long* index;
    const float* noise_in;
    float* noise;
    unsigned* words;
};

struct FwtUnfoldArgs {
    MftFwtGradJob job[FWT_MAX_LAYERS];
    int n, groups, ld;
    const float* noise;
};

// F.softplus(x, beta=100) with torch's threshold: x where 100 x > 20
__device__ __forceinline__ float softplus100(float x) {
    const double t = 100.0 * (double)x;
    return t > 20.0 ? x : (float)(log1p(exp(t)) / 100.0);
}

__global__ __launch_bounds__(FWT_FOLD_THREADS) void fwt_draw_fold_kernel(FwtFoldArgs a) {
    const unsigned long long idx = *a.index;
    __syncthreads();                                   // every thread holds the index before thread 0 replaces it
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
    const unsigned i2 = (unsigned)idx, i3 = (unsigned)(idx >> 32);
    // phase 1: the normals of every (group, layer, channel) into the noise buffer
#pragma unroll 1
    for (int l = 0; l < a.n; ++l) {
        const int C = a.job[l].C, col0 = a.job[l].col;
        const int total = a.groups * C;
        for (int i = threadIdx.x; i < total; i += FWT_FOLD_THREADS) {
            const int g = i / C, col = col0 + (i - g * C);
            const long long at = (long long)g * 2 * a.ld + col;
            float ng, nb;
            if (a.noise_in) {
                ng = a.noise_in[at];
                nb = a.noise_in[at + a.ld];
            } else {
                unsigned w0, w1;
                philox4x32_10((unsigned)col, (unsigned)g, i2, i3, k0, k1, w0, w1);
                if (a.words) {
                    a.words[at] = w0;
                    a.words[at + a.ld] = w1;
                }
                const double u1 = ((double)(w0 >> 8) + 0.5) * (1.0 / 16777216.0);
                const double u2 = ((double)(w1 >> 8) + 0.5) * (1.0 / 16777216.0);
                const double r = sqrt(-2.0 * log(u1));
                ng = (float)(r * cospi(2.0 * u2));
                nb = (float)(r * sinpi(2.0 * u2));
            }
            a.noise[at] = ng;
            a.noise[at + a.ld] = nb;
        }
    }
    // phase 2: fold.  Each thread reads back exactly the entries it wrote itself (same l, same i): no barrier is needed
#pragma unroll 1
    for (int l = 0; l < a.n; ++l) {
        const MftFwtJob jb = a.job[l];
        const int total = a.groups * jb.C;
        for (int i = threadIdx.x; i < total; i += FWT_FOLD_THREADS) {
            const int g = i / jb.C, c = i - g * jb.C;
            const long long at = (long long)g * 2 * a.ld + jb.col + c;
            const float ng = a.noise[at], nb = a.noise[at + a.ld];
            const float gm = __builtin_fmaf(ng, softplus100(jb.gamma[c]), 1.f);
            const float bt = nb * softplus100(jb.beta[c]);
            jb.gm[i] = gm;
            jb.w_fold[i] = gm * jb.w[c];
            jb.b_fold[i] = __builtin_fmaf(gm, jb.b[c], bt);
        }
    }
    if (threadIdx.x == 0) *a.index = idx + 1;
}

// one thread per (layer, channel); the sums walk the groups in group order (no atomics: reruns are bit-identical)
__global__ __launch_bounds__(FWT_UNFOLD_THREADS) void fwt_unfold_kernel(FwtUnfoldArgs a) {
    const MftFwtGradJob& jb = a.job[blockIdx.y];
    const int c = blockIdx.x * FWT_UNFOLD_THREADS + threadIdx.x;
    if (c >= jb.C) return;
    const float w = jb.w[c], b = jb.b[c];
    float sw = 0.f, sb = 0.f, sg = 0.f, st = 0.f;
    for (int g = 0; g < a.groups; ++g) {
        const int i = g * jb.C + c;
        const long long at = (long long)g * 2 * a.ld + jb.col + c;
        const float gm = jb.gm[i], dwf = jb.dw_fold[i], dbf = jb.db_fold[i];
        sw = __builtin_fmaf(gm, dwf, sw);
        sb = __builtin_fmaf(gm, dbf, sb);
        sg = __builtin_fmaf(a.noise[at], __builtin_fmaf(w, dwf, b * dbf), sg);
        st = __builtin_fmaf(a.noise[at + a.ld], dbf, st);
    }
    jb.dw[c] = sw;
    jb.db[c] = sb;
    // d softplus(x, beta=100) / dx = sigmoid(100 x) (1 beyond torch's threshold, where sigmoid(20) differs from 1 by 2e-9)
    if (jb.dgamma) jb.dgamma[c] = sg / (1.f + expf(-100.f * jb.gamma[c]));
    if (jb.dbeta) jb.dbeta[c] = st / (1.f + expf(-100.f * jb.beta[c]));
}

}  // namespace

extern "C" int mft_fwt_draw_fold(const MftFwtJob* jobs, int n_layers, int groups, int ld, unsigned long long seed,
                                 unsigned long long* index, const float* noise_in, float* noise, unsigned* words, void* stream) {
    if (jobs == nullptr || n_layers < 1 || n_layers > FWT_MAX_LAYERS || groups < 1 || ld < 1 || index == nullptr || noise == nullptr)
        return MFT_EINVAL;
    FwtFoldArgs a = {};
    for (int l = 0; l < n_layers; ++l) {
        const MftFwtJob& jb = jobs[l];
        if (jb.C < 1 || jb.C > FWT_MAX_C || jb.col < 0 || jb.col + jb.C > ld || (long long)groups * jb.C > 0x7fffffffLL || !jb.w || !jb.b ||
            !jb.gamma || !jb.beta || !jb.w_fold || !jb.b_fold || !jb.gm)
            return MFT_EINVAL;
        a.job[l] = jb;
    }
    a.n = n_layers; a.groups = groups; a.ld = ld; a.seed = seed; a.index = index; a.noise_in = noise_in; a.noise = noise; a.words = words;
    hipLaunchKernelGGL(fwt_draw_fold_kernel, dim3(1), dim3(FWT_FOLD_THREADS), 0, (hipStream_t)stream, a);
    return mft_launch_status();
}

extern "C" int mft_fwt_unfold(const MftFwtGradJob* jobs, int n_layers, int groups, int ld, const float* noise, void* stream) {
    if (jobs == nullptr || n_layers < 1 || n_layers > FWT_MAX_LAYERS || groups < 1 || ld < 1 || noise == nullptr) return MFT_EINVAL;
    FwtUnfoldArgs a = {};
    int cmax = 0;
    for (int l = 0; l < n_layers; ++l) {
        const MftFwtGradJob& jb = jobs[l];
        if (jb.C < 1 || jb.C > FWT_MAX_C || jb.col < 0 || jb.col + jb.C > ld || (long long)groups * jb.C > 0x7fffffffLL || !jb.w || !jb.b ||
            !jb.gamma || !jb.beta || !jb.gm || !jb.dw_fold || !jb.db_fold || !jb.dw || !jb.db)
            return MFT_EINVAL;
        a.job[l] = jb;
        cmax = jb.C > cmax ? jb.C : cmax;
    }
    a.n = n_layers; a.groups = groups; a.ld = ld; a.noise = noise;
    hipLaunchKernelGGL(fwt_unfold_kernel, dim3(cdiv(cmax, FWT_UNFOLD_THREADS), n_layers), dim3(FWT_UNFOLD_THREADS), 0, (hipStream_t)stream, a);
    return mft_launch_status();
}
