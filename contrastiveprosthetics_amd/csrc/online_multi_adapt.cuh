// Adaptive multi-stream online decoding (include/cpnative.h, cp_online_multi_adapt_*): the streams of online_multi.cuh with
// the BatchNorms of online_adapt.cuh kept unfolded.  One model's unfolded weights serve S <= 256 streams; each stream keeps
// its own OlState, head (alpha, eps) and float64 statistics, and the rows of all streams run through one chain of twelve
// launches per push, whatever S is:
//   olm_frontend_kernel    as for the folded multi-stream form (OlmMeta[s]: row0, M_s)
//   olam_conv_bn_kernel    BN1: grid S x 64 threads; workgroup s runs ola_conv_bn_run over its M_s rows from row0_s with its
//                          own statistics and writes conv2's operand (12 rows per window)
//   ola_gemm_kernel        conv2 as one GEMM over the 12 R packed rows (rows are independent)
//   olam_conv_bn_kernel    BN2 scan -> fc1's operand
//   olam_fc_kernel x 7     fc1..fc7: grid 512 / 16 feature tiles x row blocks.  Workgroup (f, b) owns the streams whose first
//                          row falls in row block b; it runs them in batches of consecutive streams of at most OL_MAXM rows:
//                          ola_fc_gemm of the batch's rows into LDS, one ola_fc_scan per (stream, feature), ola_fc_store
//   olm_tail_kernel        as for the folded multi-stream form, on the unfolded projection with a zero bias
// Every per-row and per-stream value goes through the device functions of the single-stream adaptive chain, and the scans
// run each stream's windows in order with its own statistics, so every stream's outputs and statistics are bit-identical to
// those of its own cp_online_adapt_* workspace fed the same chunks.
#pragma once
#include "online_adapt.cuh"
#include "online_multi.cuh"

constexpr int OLAM_STATS = 9 * 2 * OLA_F;                      // doubles of one stream's statistics

struct OlamConvBnArgs {
    OlaConvBnArgs a;                     // a.x, a.pre, a.out: packed row 0; a.bn.stats, a.bn.head: stream 0's
    const OlmMeta* meta;
};

// BN1 or BN2, grid S: workgroup s scans stream s's rows
template <typename T>
__global__ __launch_bounds__(64) void olam_conv_bn_kernel(OlamConvBnArgs p) {
    const int s = blockIdx.x;
    const OlmMeta mt = p.meta[s];
    if (mt.m <= 0) return;
    OlaConvBnArgs a = p.a;
    const size_t es = sizeof(T);
    if (a.conv1) {
        a.x += (size_t)mt.row0 * OL_C;
        a.out = (unsigned char*)a.out + (size_t)mt.row0 * OL_C * OL_CONV_K * es;
    } else {
        a.pre += (size_t)mt.row0 * OL_C * 64;
        a.out = (unsigned char*)a.out + (size_t)mt.row0 * OL_C * 64 * es;
    }
    a.bn.stats += (size_t)s * OLAM_STATS;
    a.bn.head += s;
    ola_conv_bn_run<T>(a, mt.m);
}

struct OlamFcArgs {
    OlaGemmArgs g;                       // g.l.act, g.l.out: packed row 0; g.bn.stats, g.bn.head: stream 0's
    const OlmMeta* meta;
    int n_streams, rows_per_block;
};

// fc1..fc7 for all streams: grid (512 / 16, row blocks)
template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olam_fc_kernel(OlamFcArgs p) {
    __shared__ OlTileLds<T> L;
    __shared__ float pre[OL_MAXM][17];
    __shared__ OlmMeta mt[OLM_MAXS];
    __shared__ int s_first, s_last;
    const int tid = threadIdx.x, f0 = blockIdx.x * 16;
    const int r_begin = blockIdx.y * p.rows_per_block, r_end = r_begin + p.rows_per_block;
    if (tid == 0) {
        s_first = OLM_MAXS;
        s_last = -1;
    }
    __syncthreads();
    if (tid < p.n_streams) {                 // the streams with rows that start in this block: consecutive, as row0 grows
        mt[tid] = p.meta[tid];
        if (mt[tid].m > 0 && mt[tid].row0 >= r_begin && mt[tid].row0 < r_end) {
            atomicMin(&s_first, tid);
            atomicMax(&s_last, tid);
        }
    }
    __syncthreads();
    const int first = s_first, last = s_last;
    if (first > last) return;
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)p.g.l.w, p.g.l.K, f0, wf);
    const size_t es = sizeof(T);
    for (int s = first; s <= last;) {
        const int base = mt[s].row0;
        int e = s + 1;                       // batch: streams s..e-1, at most OL_MAXM rows (one stream has at most OL_MAXM)
        while (e <= last && mt[e].row0 + mt[e].m - base <= OL_MAXM) ++e;
        const int M = mt[e - 1].row0 + mt[e - 1].m - base;
        OlaGemmArgs a = p.g;
        a.l.act = (const unsigned char*)p.g.l.act + (size_t)base * a.l.K * es;
        a.l.out = (unsigned char*)p.g.l.out + (size_t)base * a.l.ldo * es;
        ola_fc_gemm<T>(a, L, pre, f0, M, wf);
        for (int q = tid; q < (e - s) * 16; q += OL_THREADS) {
            const int j = s + (q >> 4), col = q & 15;
            if (mt[j].m <= 0) continue;
            OlaBn bn = p.g.bn;
            bn.stats += (size_t)j * OLAM_STATS;
            bn.head += j;
            ola_fc_scan(bn, pre + (mt[j].row0 - base), f0, col, mt[j].m);
        }
        __syncthreads();
        ola_fc_store<T>(a, pre, f0, M);
        __syncthreads();                     // the next batch's GEMM writes pre
        s = e;
    }
}

// cp_online_multi_adapt_prepare (grid 9 x S) and cp_online_multi_adapt_reset_statistics (grid 9 x 1, first = the stream):
// gamma, beta, conv1 and every stream's eps (and alpha, if set_alpha) once (none of them when reset); the statistics of
// streams first.. to the running statistics, or (mean all NULL) kept, or (zero) to zero
struct OlamInitArgs {
    const float* g[9];
    const float* beta[9];
    const float* mean[9];
    const float* var[9];
    const float* c1w;         // NULL: gamma, beta, conv1 and eps stay
    const float* c1b;
    float* gb;
    double* stats;            // stream 0's
    float* c1w_d;
    float* c1b_d;
    OlaHead* heads;
    double eps;
    int first, zero, set_alpha;
    double alpha[OLM_MAXS];   // set_alpha: stream s's alpha
};
static_assert(sizeof(OlamInitArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(512) void olam_init_kernel(OlamInitArgs a) {
    const int l = blockIdx.x, s = a.first + blockIdx.y, c = threadIdx.x, C = l < 2 ? 64 : 512;
    double* st = a.stats + (size_t)s * OLAM_STATS;
    if (c < C && a.c1w && blockIdx.y == 0) {
        a.gb[(l * 2) * OLA_F + c] = a.g[l][c];
        a.gb[(l * 2 + 1) * OLA_F + c] = a.beta[l][c];
    }
    if (a.mean[l]) {
        if (c < C) {
            st[(l * 2) * OLA_F + c] = (double)a.mean[l][c];
            st[(l * 2 + 1) * OLA_F + c] = (double)a.var[l][c];
        }
    } else if (a.zero) {
        st[(l * 2) * OLA_F + c] = 0.0;
        st[(l * 2 + 1) * OLA_F + c] = 0.0;
    }
    if (a.c1w && l == 0 && blockIdx.y == 0 && c < 64) {
        for (int t = 0; t < 3; ++t) a.c1w_d[c * 3 + t] = a.c1w[c * 9 + 3 + t];
        a.c1b_d[c] = a.c1b[c];
    }
    if (a.c1w && l == 0 && c == 0) {
        a.heads[s].eps = a.eps;
        if (a.set_alpha) a.heads[s].alpha = a.alpha[s];
    }
}

// cp_online_multi_adapt_set_alpha
__global__ __launch_bounds__(64) void olam_set_alpha_kernel(OlaHead* head, double alpha) {
    if (threadIdx.x == 0) head->alpha = alpha;
}
