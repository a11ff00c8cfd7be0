// Class enrolment (include/cpnative.h, cp_online_*enroll*): a user's own windows -> per-class sums of z / |z| in a
// caller-owned float64 accumulator -> class rows (cosine prototypes) blended with the rows the decoder has.
//
// An accumulate call runs the windows it is given through the decoder's own encoder in chunks of <= 256 windows (whole
// 16-row tiles): the folded form through ole_layer_kernel (ol_layer_tiles with a fixed row count instead of the push's
// st->m_cur), the adaptive form through the frozen pass of the calibration (ola_conv_chain / ola_fc with OLA_FROZEN), and
// ends each chunk with
//   ole_accumulate_kernel  one workgroup: the projection tile by tile (ol_load_weights / ol_tile), z / |z| as ol_tail_run
//                          computes it, then thread (slot, dimension) walks the tile's 16 rows in order and adds the rows
//                          of its slot in float64.  Tiles, chunks and calls follow each other in window order, so every
//                          (slot, dimension) sum is one float64 add per window in window order: no atomics, no reduction
//                          across workgroups, and the accumulator does not depend on how the windows were cut into calls.
// cp_online_windows is the front end of a push alone (ol_frontend_run on a caller-owned state), and
// ole_table_kernel the blend of the accumulated directions with the prior rows.
#pragma once
#include "online_adapt.cuh"

constexpr int OLE_ACC_W = 17;            // per slot: 16 sums and the window count

// conv2 (CONV) or one fc layer of the folded form over rows 0..M-1 of a.x / a.act: ol_layer_kernel with the row count as
// an argument
template <typename T, bool CONV>
__global__ __launch_bounds__(OL_THREADS) void ole_layer_kernel(OlLayerArgs a, int M) {
    __shared__ OlTileLds<T> L;
    ol_layer_tiles<T, CONV>(a, L, blockIdx.x * 16, CONV ? (int)blockIdx.y : 0, 0, M, M);
}

// cp_online_windows: the windows of the chunk to p.X from row 0; the state's sample count moves on as in a push
template <int NB>
__global__ __launch_bounds__(256) void ole_windows_kernel(OlFrontArgs p) {
    __shared__ float xs[OL_FRONT_PIECE * OL_C];
    OlState* st = p.st;
    const long long n0 = st->n_seen;
    const int j = ol_frontend_run<NB>(p, st, p.raw, p.n, n0, p.X, nullptr, xs);       // (every thread has read n_seen)
    if (threadIdx.x == 0) {
        st->n_seen = n0 + p.n;
        st->m_cur = j;
    }
}

struct OleAccArgs {
    OlLayerArgs proj;         // act = fc7 output of the chunk [M][512], w / bias = the projection as the tail takes it
    const int32_t* slots;     // [M] slot of each window; outside 0..n_classes-1: skipped
    double* acc;              // [64][17]
    int M, n_classes;
};

template <typename T>
struct OleAccLds {
    OlTileLds<T> L;
    float zn[16][17];
    int slot[16];
};

template <typename T>
__global__ __launch_bounds__(OL_THREADS) void ole_accumulate_kernel(OleAccArgs a) {
#pragma clang fp contract(off)
    __shared__ OleAccLds<T> S;
    OlTileLds<T>& L = S.L;
    const int tid = threadIdx.x, M = a.M;
    // thread tid owns (slot, d) = (tid >> 4, tid & 15) and (32 + (tid >> 4), tid & 15); d == 0 also keeps the slot's count
    const int d = tid & 15, s0 = tid >> 4, s1 = s0 + OL_THREADS / 16;
    double sum0 = a.acc[s0 * OLE_ACC_W + d], sum1 = a.acc[s1 * OLE_ACC_W + d];
    double cnt0 = 0.0, cnt1 = 0.0;
    if (d == 0) {
        cnt0 = a.acc[s0 * OLE_ACC_W + 16];
        cnt1 = a.acc[s1 * OLE_ACC_W + 16];
    }
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)a.proj.w, 512, 0, wf);
    for (int m0 = 0; m0 < M; m0 += 16) {
        ol_tile<T, false>(a.proj, L, 512, 0, m0, M, wf);
        if (tid < 16) {                               // as ol_tail_run: z, then z / sqrtf(ss), in f32
            float z[16], ss = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                z[k] = L.red[0][tid][k] + a.proj.bias[k];
                ss += z[k] * z[k];
            }
            const float nrm = sqrtf(ss);
#pragma unroll
            for (int k = 0; k < 16; ++k) S.zn[tid][k] = z[k] / nrm;
            int sl = -1;
            if (m0 + tid < M) {
                sl = a.slots[m0 + tid];
                if (sl < 0 || sl >= a.n_classes) sl = -1;
            }
            S.slot[tid] = sl;
        }
        __syncthreads();
        for (int r = 0; r < 16; ++r) {                // the tile's windows in order
            const int sl = S.slot[r];
            if (sl == s0) {
                sum0 += (double)S.zn[r][d];
                cnt0 += 1.0;
            } else if (sl == s1) {
                sum1 += (double)S.zn[r][d];
                cnt1 += 1.0;
            }
        }
        __syncthreads();                              // zn and slot are rewritten by the next tile
    }
    a.acc[s0 * OLE_ACC_W + d] = sum0;
    a.acc[s1 * OLE_ACC_W + d] = sum1;
    if (d == 0) {
        a.acc[s0 * OLE_ACC_W + 16] = cnt0;
        a.acc[s1 * OLE_ACC_W + 16] = cnt1;
    }
}

// cp_online_enroll_table: thread c blends slot c.  With E = prior_c / |prior_c| (f32, as ol_set_classes_kernel takes it)
// and P = S_c / |S_c| (float64), the row is |prior_c| ((1 - mix) E + mix P), written as (1 - mix) prior_c + mix |prior_c| P:
// the direction the header states, at the prior's length, so that mix = 0 and a slot that is not enrolled return prior_c
// bit for bit.  A zero prior row has no direction: its row is P alone.
__global__ __launch_bounds__(64) void ole_table_kernel(const double* __restrict__ acc, int n_classes, const float* __restrict__ prior,
                                                       double mix, double min_windows, float* __restrict__ table) {
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= n_classes) return;
    float ss = 0.f;
    for (int d = 0; d < 16; ++d) ss += prior[c * 16 + d] * prior[c * 16 + d];
    const double len = (double)sqrtf(ss);
    double s2 = 0.0;
    for (int d = 0; d < 16; ++d) s2 += acc[c * OLE_ACC_W + d] * acc[c * OLE_ACC_W + d];
    const double sn = sqrt(s2);
    const bool enrolled = acc[c * OLE_ACC_W + 16] >= min_windows && sn > 0.0;
    for (int d = 0; d < 16; ++d) {
        const float e = prior[c * 16 + d];
        float v = e;
        if (enrolled) {
            const double p = acc[c * OLE_ACC_W + d] / sn;
            v = len > 0.0 ? (float)((1.0 - mix) * (double)e + mix * (len * p)) : (float)p;
        }
        table[c * 16 + d] = v;
    }
}
