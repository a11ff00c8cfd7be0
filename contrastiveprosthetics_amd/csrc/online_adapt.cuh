// Adaptive online decoding (include/cpnative.h, cp_online_adapt_*): the online decoder of online.cuh with BatchNorm kept
// unfolded and its statistics (float64 mu, v per BN channel) held in the workspace.  They come from the model's running
// statistics, or from a calibration recording (AdaBN), and a push may track the stream with rate alpha:
//     y = gamma (x - mu) / sqrt(v + eps) + beta   with the statistics before window t, then
//     d = m - mu,  mu <- mu + alpha d,  v <- (1 - alpha)(v + alpha d^2) + alpha w
// (m, w: mean and biased variance of the window's P values of the channel; P = 12 for BN1 and BN2, 1 for BN3..BN9).
//
// A push is a chain of twelve launches on one stream:
//   ol_frontend_kernel     as for the folded form
//   ola_conv_bn_kernel     BN1: conv1 per channel, the scan over the push's windows in order, and the normalised output as
//                          conv2's operand: rows (window, position), 192 columns (tap-major), zeros where conv2 pads
//   ola_gemm_kernel        conv2 as a GEMM over those rows (f32 pre-BN output, ReLU applied)
//   ola_conv_bn_kernel     BN2 scan -> fc1's operand (position-major)
//   ola_fc_kernel x 7      fc1..fc7: each workgroup owns 16 features for all rows; the pre-BN outputs stay in LDS and 16
//                          threads run the scan of their feature over the windows in order
//   ol_tail_kernel         as for the folded form, on the unfolded projection with a zero bias
// The GEMMs sum their tiles as ol_tile does, and each scan is serial in float64 over windows in stream order, so every
// output and the statistics after a push are bit-identical for any chunking.
//
// Calibration (cp_online_adapt_calibrate) runs the same kernels layer by layer over the calibration windows in chunks of
// <= 256: an OLA_ACC pass merges per-window (n, mean, M2) in float64 into an accumulator in a fixed order (Chan et al.) and
// the last chunk writes mu = mean, v = M2 / n; then an OLA_FROZEN pass normalises the chunks with those statistics into the
// next layer's input.
#pragma once
#include "online.cuh"

constexpr int OLA_F = 512;               // stride of one BN's channels in the statistics block
constexpr int OLA_TRACK = 0;             // push: normalise, then update with the workspace's alpha
constexpr int OLA_ACC = 1;               // calibration: accumulate (n, mean, M2); no output
constexpr int OLA_FROZEN = 2;            // calibration: normalise with the statistics as they are; no update

struct OlaHead {                          // in the workspace, written by cp_online_adapt_prepare
    double alpha, eps;
};

struct OlaBn {
    double* stats;            // [2][512]: mu, v of this BN
    double* acc;              // OLA_ACC: [3][512]: n, mean, M2
    const float* gamma;       // [512]
    const float* beta;
    const OlaHead* head;
    int mode, first, last;    // first: the accumulator starts at zero; last: finalise into stats
};

__device__ __forceinline__ void ola_merge(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
#pragma clang fp contract(off)
    const double nn = n + nb, d = mb - mean;
    mean = mean + d * (nb / nn);
    m2 = (m2 + m2b) + d * d * (n * nb / nn);
    n = nn;
}

__device__ __forceinline__ void ola_update(double& mu, double& v, double m, double w, double alpha) {
#pragma clang fp contract(off)
    const double d = m - mu;
    mu = mu + alpha * d;
    v = (1.0 - alpha) * (v + alpha * d * d) + alpha * w;
}

// One BN channel's state in registers for a scan: the statistics (normalise / update) or the accumulator (OLA_ACC)
struct OlaChan {
    double mu, v, n, mean, m2, alpha, eps, g, b;
    __device__ __forceinline__ void load(const OlaBn& bn, int c) {
        mu = bn.stats[c];
        v = bn.stats[OLA_F + c];
        alpha = bn.mode == OLA_TRACK ? bn.head->alpha : 0.0;
        eps = bn.head->eps;
        g = (double)bn.gamma[c];
        b = (double)bn.beta[c];
        n = mean = m2 = 0.0;
        if (bn.mode == OLA_ACC && !bn.first) {
            n = bn.acc[c];
            mean = bn.acc[OLA_F + c];
            m2 = bn.acc[2 * OLA_F + c];
        }
    }
    __device__ __forceinline__ double scale() const { return g / sqrt(v + eps); }
    __device__ __forceinline__ float norm(float x, double s) const { return (float)(((double)x - mu) * s + b); }
    __device__ __forceinline__ void store(const OlaBn& bn, int c) const {
        if (bn.mode == OLA_ACC) {
            bn.acc[c] = n;
            bn.acc[OLA_F + c] = mean;
            bn.acc[2 * OLA_F + c] = m2;
            if (bn.last) {
                bn.stats[c] = mean;
                bn.stats[OLA_F + c] = m2 / n;
            }
        } else if (bn.mode == OLA_TRACK) {
            bn.stats[c] = mu;
            bn.stats[OLA_F + c] = v;
        }
    }
};

struct OlaConvBnArgs {
    const float* x;           // BN1: normalised windows [M][12]
    const float* c1w;         // BN1: conv1 taps [64][3]
    const float* c1b;         // BN1: conv1 bias [64]
    const float* pre;         // BN2: conv2 output [M][12 * 64], ReLU applied
    void* out;                // BN1: conv2 operand [M * 12][192]; BN2: fc1 operand [M][12 * 64]; compute dtype
    const OlState* st;
    int m_fixed;              // >= 0: the row count (calibration); < 0: the push's st->m_cur
    int conv1;                // 1: BN1, 0: BN2
    OlaBn bn;
};

// BN1 or BN2 over M >= 1 windows from row 0 of a.x / a.pre / a.out with the statistics of a.bn: thread c (64 threads) runs
// channel c, serial over the windows
template <typename T>
__device__ __forceinline__ void ola_conv_bn_run(const OlaConvBnArgs& a, int M) {
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    OlaChan s;
    s.load(a.bn, c);
    float w1[3] = {0.f, 0.f, 0.f}, b1 = 0.f;
    if (a.conv1) {
        for (int t = 0; t < 3; ++t) w1[t] = a.c1w[c * 3 + t];
        b1 = a.c1b[c];
    }
    T* out = (T*)a.out;
    for (int t = 0; t < M; ++t) {
        float u[OL_C];
        if (a.conv1) {                                // as ol_tile stages conv1 for the folded form
            const float* xr = a.x + (size_t)t * OL_C;
#pragma unroll
            for (int p = 0; p < OL_C; ++p) {
                float acc = b1;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int q = p + k - 1;
                    if (q >= 0 && q < OL_C) acc = fmaf(w1[k], xr[q], acc);
                }
                u[p] = fmaxf(acc, 0.f);
            }
        } else {
#pragma unroll
            for (int p = 0; p < OL_C; ++p) u[p] = a.pre[(size_t)t * OL_C * 64 + p * 64 + c];
        }
        double sum = 0.0;
#pragma unroll
        for (int p = 0; p < OL_C; ++p) sum += (double)u[p];
        const double m = sum / (double)OL_C;
        double ss = 0.0;
#pragma unroll
        for (int p = 0; p < OL_C; ++p) {
            const double d = (double)u[p] - m;
            ss += d * d;
        }
        if (a.bn.mode == OLA_ACC) {
            ola_merge(s.n, s.mean, s.m2, (double)OL_C, m, ss);
            continue;
        }
        const double sc = s.scale();
        float y[OL_C];
#pragma unroll
        for (int p = 0; p < OL_C; ++p) y[p] = s.norm(u[p], sc);
        if (a.conv1) {                                // row (t, pos), column kw * 64 + c = input position pos + kw - 1
#pragma unroll
            for (int pos = 0; pos < OL_C; ++pos)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int q = pos + kw - 1;
                    out[((size_t)t * OL_C + pos) * OL_CONV_K + kw * 64 + c] = ol_cvt<T>(q >= 0 && q < OL_C ? y[q] : 0.f);
                }
        } else {
#pragma unroll
            for (int p = 0; p < OL_C; ++p) out[(size_t)t * OL_C * 64 + p * 64 + c] = ol_cvt<T>(y[p]);
        }
        ola_update(s.mu, s.v, m, ss / (double)OL_C, s.alpha);
    }
    s.store(a.bn, c);
}

template <typename T>
__global__ __launch_bounds__(64) void ola_conv_bn_kernel(OlaConvBnArgs a) {
    const int M = a.m_fixed >= 0 ? a.m_fixed : a.st->m_cur;
    if (M <= 0) return;
    ola_conv_bn_run<T>(a, M);
}

struct OlaGemmArgs {
    OlLayerArgs l;            // act [rows][K], w [F][K] compute dtype, bias [F], out: see the kernels
    int m_fixed;              // as OlaConvBnArgs
    int rows_per_window;      // conv2: 12
    OlaBn bn;
};

// conv2: out f32 [rows][F] = relu(A W^T + b), rows = 12 M; grid (F / 16, row-tile groups)
template <typename T>
__global__ __launch_bounds__(OL_THREADS) void ola_gemm_kernel(OlaGemmArgs a) {
#pragma clang fp contract(off)
    __shared__ OlTileLds<T> L;
    const int M = a.m_fixed >= 0 ? a.m_fixed : a.l.st->m_cur;
    if (M <= 0) return;
    const int rows = M * a.rows_per_window, f0 = blockIdx.x * 16, tid = threadIdx.x;
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)a.l.w, a.l.K, f0, wf);
    for (int m0 = blockIdx.y * 16; m0 < rows; m0 += 16 * gridDim.y) {
        ol_tile<T, false>(a.l, L, a.l.K, 0, m0, rows, wf);
        if (tid < 256) {
            const int row = tid >> 4, col = tid & 15;
            if (m0 + row < rows)
                ((float*)a.l.out)[(size_t)(m0 + row) * a.l.F + f0 + col] = fmaxf(L.red[0][row][col] + a.l.bias[f0 + col], 0.f);
        }
    }
}

// fc1..fc7, in three steps that the single-stream and the multi-stream kernels share.
// M (1..OL_MAXM) rows of a.l.act from row 0: relu(A W^T + b) for features f0..f0+15 into pre.  Ends behind a barrier.
template <typename T>
__device__ __forceinline__ void ola_fc_gemm(const OlaGemmArgs& a, OlTileLds<T>& L, float (*pre)[17], int f0, int M,
                                            const uint4 (&wf)[OL_MAXCH][OL_KC * (int)sizeof(T) / 64]) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    for (int m0 = 0; m0 < M; m0 += 16) {
        ol_tile<T, false>(a.l, L, a.l.K, 0, m0, M, wf);
        if (tid < 256) {
            const int row = tid >> 4, col = tid & 15;
            if (m0 + row < M) pre[m0 + row][col] = fmaxf(L.red[0][row][col] + a.l.bias[f0 + col], 0.f);
        }
    }
    __syncthreads();
}

// One thread: the BN scan of feature f0 + col over the M rows pre[0..M-1][col] with the statistics of bn; OLA_TRACK /
// OLA_FROZEN leave the normalised values in pre
__device__ __forceinline__ void ola_fc_scan(const OlaBn& bn, float (*pre)[17], int f0, int col, int M) {
#pragma clang fp contract(off)
    const int f = f0 + col;
    OlaChan s;
    s.load(bn, f);
    if (bn.mode == OLA_ACC) {
        for (int t = 0; t < M; ++t) ola_merge(s.n, s.mean, s.m2, 1.0, (double)pre[t][col], 0.0);
    } else {
        double sc = s.scale();
        for (int t = 0; t < M; ++t) {
            const float x = pre[t][col];
            pre[t][col] = s.norm(x, sc);
            if (s.alpha != 0.0) {
                ola_update(s.mu, s.v, (double)x, 0.0, s.alpha);
                sc = s.scale();
            }
        }
    }
    s.store(bn, f);
}

// The M normalised rows of pre into a.l.out from row 0 (ldo a.l.ldo) in the compute dtype
template <typename T>
__device__ __forceinline__ void ola_fc_store(const OlaGemmArgs& a, float (*pre)[17], int f0, int M) {
    for (int e = threadIdx.x; e < M * 16; e += OL_THREADS) {
        const int row = e >> 4, col = e & 15;
        ((T*)a.l.out)[(size_t)row * a.l.ldo + f0 + col] = ol_cvt<T>(pre[row][col]);
    }
}

// fc1..fc7: relu(A W^T + b) for 16 features and all rows into LDS, then the BN scan of each feature over the windows in
// order; OLA_TRACK / OLA_FROZEN write the normalised rows [M][512] in the compute dtype.  Grid 512 / 16.
template <typename T>
__global__ __launch_bounds__(OL_THREADS) void ola_fc_kernel(OlaGemmArgs a) {
    __shared__ OlTileLds<T> L;
    __shared__ float pre[OL_MAXM][17];
    const int M = a.m_fixed >= 0 ? a.m_fixed : a.l.st->m_cur;
    if (M <= 0) return;
    const int f0 = blockIdx.x * 16, tid = threadIdx.x;
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)a.l.w, a.l.K, f0, wf);
    ola_fc_gemm<T>(a, L, pre, f0, M, wf);
    if (tid < 16) ola_fc_scan(a.bn, pre, f0, tid, M);
    if (a.bn.mode == OLA_ACC) return;
    __syncthreads();
    ola_fc_store<T>(a, pre, f0, M);
}

// ---- cp_online_adapt_prepare: the model's parameters into the workspace, unfolded ----------------------------------------
struct OlaCopyArgs {
    const float* W;           // source weight (row-major as the state_dict holds it)
    const float* b;           // source bias (NULL: none)
    void* Wd;                 // [F][K] compute dtype
    float* bd;                // [F]
    int K;                    // destination row length
    int mode;                 // 0: plain, 1: fc1 (columns o*12+w -> w*64+o), 2: conv2 (taps [o][i][1][kw] -> [o][kw*64+i])
};

template <typename T>
__global__ __launch_bounds__(256) void ola_copy_kernel(OlaCopyArgs a) {
    const int f = blockIdx.x;
    for (int k = threadIdx.x; k < a.K; k += 256) {
        int src;
        if (a.mode == 0) src = k;
        else if (a.mode == 1) src = (k & 63) * 12 + (k >> 6);
        else src = (k & 63) * 9 + 3 + (k >> 6);
        ((T*)a.Wd)[(size_t)f * a.K + k] = ol_cvt<T>(a.W[(size_t)f * (a.mode == 2 ? 576 : a.K) + src]);
    }
    if (threadIdx.x == 0 && a.bd) a.bd[f] = a.b ? a.b[f] : 0.f;
}

struct OlaBnInitArgs {
    const float* g[9];
    const float* beta[9];
    const float* mean[9];     // all NULL: the statistics stay as they are
    const float* var[9];
    const float* c1w;         // conv1 source [64][1][3][3]
    const float* c1b;
    float* gb;                // [9][2][512]
    double* stats;            // [9][2][512]
    float* c1w_d;             // [64][3]
    float* c1b_d;
    OlaHead* head;
    double alpha, eps;
};

// grid 9 (one BN each), 512 threads
__global__ __launch_bounds__(512) void ola_bn_init_kernel(OlaBnInitArgs a) {
    const int l = blockIdx.x, c = threadIdx.x, C = l < 2 ? 64 : 512;
    if (c < C) {
        a.gb[(l * 2) * OLA_F + c] = a.g[l][c];
        a.gb[(l * 2 + 1) * OLA_F + c] = a.beta[l][c];
        if (a.mean[l]) {
            a.stats[(l * 2) * OLA_F + c] = (double)a.mean[l][c];
            a.stats[(l * 2 + 1) * OLA_F + c] = (double)a.var[l][c];
        }
    }
    if (l == 0 && c < 64) {
        for (int t = 0; t < 3; ++t) a.c1w_d[c * 3 + t] = a.c1w[c * 9 + 3 + t];
        a.c1b_d[c] = a.c1b[c];
    }
    if (l == 0 && c == 0) {
        a.head->alpha = a.alpha;
        a.head->eps = a.eps;
    }
}
