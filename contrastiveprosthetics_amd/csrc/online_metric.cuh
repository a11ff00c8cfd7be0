// User metric (include/cpnative.h, cp_online_metric_*): within-class whitening of the 16-d embedding.  Every stage of the
// personalisation chain compares a window with a class row by a plain cosine, which weighs all sixteen directions alike, while
// a person's windows spread along a few shared directions (force, fatigue, arm position).  The pooled within-class scatter of a
// cued recording, shrunk towards the identity, gives a 16 x 16 lower-triangular A per user with A Sw A^T = I; a window e becomes
// A e / |A e| and is compared with class rows fitted in that space.  fit_reference, apply_reference and stage_reference of
// contrastiveprosthetics_amd/metric.py are the definitions; the device equals them in every integer and bit.
//
//   om_moments_kernel   grid n_classes, one wave per class (the shape of op_fit_kernel / oh_sums_kernel).  Windows come 64 at a
//                       time, one per lane: the lane tests its window (slot, use, all 16 components finite) and puts its 16
//                       floats into LDS behind a constant 1; the class's windows, found by one ballot, are walked in window
//                       order.  The 16 sums and 136 products of a class are spread over the lanes, accumulator a on lane
//                       a % 64 (three or fewer per lane), each the float64 product of two LDS entries (a sum: entry x 1), which
//                       is exact, and one float64 add per window.
//   om_factor_kernel    grid n_shrinks, one wave per shrink value.  Every wave pools the scatter itself, entry (i, j) on the
//                       lane the moments kernel gave it, over the fitted classes in slot order; the 16 x 16 matrices then live
//                       in LDS.  Cholesky runs column by column: lane j forms the pivot, then lane i > j the element below it,
//                       whose k-sum is serial and which depends on no other element of its column; that is the row-wise
//                       order of the definition element by element.  The inverse is independent per column: lane j solves
//                       column j by forward substitution.
//   om_apply_kernel     one thread per window, A in LDS (every lane reads one address: a broadcast).
//   om_push_kernel      the stage: grid n_streams, one wave each.  The push's embeddings (<= 256 x 64 B) are staged in LDS and
//                       transformed there in place, one window per lane; then the windows are walked in order: lane k's logit
//                       against its unit row, the first maximum as a wave maximum of (value, 255 - lane) keys (ot_key), the
//                       decoders' vote ring (ol_vote_step), as oh_score_kernel does.
//   om_set_kernel, om_reset_kernel   one wave per stream.
// Everything is integer, single f32 or single f64 operations with floating-point contraction off, no atomics.  Every value
// read from the device is checked before it is an index: a slot is only compared with the class, a count only with
// min_windows, a stream's K / row0 / m / ring position against the limits; ring entries are only compared with a lane.
#pragma once
#include "online_prototypes.cuh"

constexpr int OM_MAXK = 64;              // class slots (CP_ONLINE_MAX_CLASSES)
constexpr int OM_D = 16;                 // embedding width (CP_D_E)
constexpr int OM_PAIRS = OM_D * (OM_D + 1) / 2;          // 136 entries (i <= j), i-major
constexpr int OM_MOMENTS = OM_D + OM_PAIRS;              // 152 doubles per class (CP_ONLINE_METRIC_MOMENTS): S[16], P[136]
constexpr int OM_MAX_SHRINKS = 64;       // CP_ONLINE_METRIC_MAX_SHRINKS
constexpr int OM_MAXM = 256;             // rows of one stream per push (CP_ONLINE_MAX_WINDOWS)
constexpr int OM_LD = OM_D + 1;          // LDS row: 16 components and a constant 1 (an odd stride: no bank conflict by row)

// accumulator a (0..151) reads the LDS entries (i, j): a < 16 is the sum S[a] = e[a] x 1, the others the pairs in i-major order
__device__ __forceinline__ void om_entry(int a, int& i, int& j) {
    if (a < OM_D) {
        i = a;
        j = OM_D;
        return;
    }
    int rem = a - OM_D;
    i = 0;
    while (rem >= OM_D - i) {
        rem -= OM_D - i;
        ++i;
    }
    j = i + rem;
}

// grid K, 64 threads: moments[c][0..151] and counts[c] of class slot c = blockIdx.x
__global__ __launch_bounds__(64) void om_moments_kernel(const float* __restrict__ emb, long long n_rows, const int32_t* __restrict__ slot,
                                                        const uint8_t* __restrict__ use, double* __restrict__ moments,
                                                        long long* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ float es[64 * OM_LD];
    const int lane = threadIdx.x, c = blockIdx.x;
    int i0, j0, i1, j1, i2, j2;
    om_entry(lane, i0, j0);
    om_entry(lane + 64, i1, j1);
    const bool third = lane + 128 < OM_MOMENTS;
    om_entry(third ? lane + 128 : lane, i2, j2);
    es[lane * OM_LD + OM_D] = 1.f;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    long long n = 0;
    for (long long base = 0; base < n_rows; base += 64) {
        const long long w = base + lane;
        bool mine = false;
        float e[OM_D];
#pragma unroll
        for (int d = 0; d < OM_D; ++d) e[d] = 0.f;
        if (w < n_rows && slot[w] == c && (use ? use[w] != 0 : true)) {
            const float4* src = (const float4*)(emb + (size_t)w * OM_D);
            mine = true;
#pragma unroll
            for (int q = 0; q < OM_D / 4; ++q) {
                const float4 v = src[q];
                e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int d = 0; d < OM_D; ++d) mine = mine && isfinite(e[d]);
        }
        __builtin_amdgcn_wave_barrier();                       // (one wave: the block before has read es)
        if (mine) {
#pragma unroll
            for (int d = 0; d < OM_D; ++d) es[lane * OM_LD + d] = e[d];
        }
        __builtin_amdgcn_wave_barrier();
        unsigned long long todo = __ballot(mine);
        n += __popcll(todo);
        while (todo) {                                         // the class's windows of this block in window order
            const int j = og_first(todo);
            todo &= todo - 1ull;
            const float* r = es + j * OM_LD;
            a0 += (double)r[i0] * (double)r[j0];
            a1 += (double)r[i1] * (double)r[j1];
            a2 += (double)r[i2] * (double)r[j2];
        }
    }
    double* out = moments + (size_t)c * OM_MOMENTS;
    out[lane] = a0;
    out[lane + 64] = a1;
    if (third) out[lane + 128] = a2;
    if (lane == 0) counts[c] = n;
}

struct OmFactorArgs {
    const double* moments;               // [K][152]
    const long long* counts;             // [K]
    int K, min_windows, n_shrinks;
    double shrinks[OM_MAX_SHRINKS];      // within [0, 1], checked on the host
    float* A;                            // [n_shrinks][16][16]
    uint8_t* valid;                      // [n_shrinks]
};

// the pooled entry of accumulator a (>= 16) over the fitted classes in slot order, before the division by N - C
__device__ __forceinline__ double om_pool(const OmFactorArgs& a, int acc, int i, int j) {
#pragma clang fp contract(off)
    double sw = 0.0;
    for (int c = 0; c < a.K; ++c) {
        const long long n = a.counts[c];
        if (n < (long long)a.min_windows) continue;            // (uniform over the wave)
        const double* m = a.moments + (size_t)c * OM_MOMENTS;
        double t = m[i] * m[j];
        t = t / (double)n;
        sw += m[acc] - t;
    }
    return sw;
}

// grid n_shrinks, 64 threads
__global__ __launch_bounds__(64) void om_factor_kernel(OmFactorArgs a) {
#pragma clang fp contract(off)
    __shared__ double B[OM_D * OM_LD], L[OM_D * OM_LD], Ai[OM_D * OM_LD];
    const int lane = threadIdx.x, t = blockIdx.x;
    const double lam = a.shrinks[t];
    long long N = 0, C = 0;
    for (int c = 0; c < a.K; ++c) {
        const long long n = a.counts[c];
        if (n >= (long long)a.min_windows) {
            N += n;
            ++C;
        }
    }
    bool ok = N - C >= 1;
    if (ok) {                                                  // (uniform over the wave)
        const double den = (double)(N - C);
        int i, j;
        om_entry(lane + OM_D, i, j);                           // 136 entries: lanes 0..63, then 0..63, then 0..7
        const double s0 = om_pool(a, lane + OM_D, i, j) / den;
        B[i * OM_LD + j] = s0;
        B[j * OM_LD + i] = s0;
        om_entry(lane + OM_D + 64, i, j);
        const double s1 = om_pool(a, lane + OM_D + 64, i, j) / den;
        B[i * OM_LD + j] = s1;
        B[j * OM_LD + i] = s1;
        if (lane + OM_D + 128 < OM_MOMENTS) {
            om_entry(lane + OM_D + 128, i, j);
            const double s2 = om_pool(a, lane + OM_D + 128, i, j) / den;
            B[i * OM_LD + j] = s2;
            B[j * OM_LD + i] = s2;
        }
        __builtin_amdgcn_wave_barrier();
        double tr = 0.0;
        for (int d = 0; d < OM_D; ++d) tr += B[d * OM_LD + d];
        const double s = tr / 16.0;
        ok = isfinite(s) && s > 0.0;
        __builtin_amdgcn_wave_barrier();
        if (ok) {
            const double keep = 1.0 - lam;
            for (int e = lane; e < OM_D * OM_D; e += 64) {     // B = (1 - lam) (Sw / s) + (lam on the diagonal, 0 off it)
                const int r = e >> 4, q = e & 15;
                const double v = keep * (B[r * OM_LD + q] / s);
                B[r * OM_LD + q] = v + (r == q ? lam : 0.0);
            }
            __builtin_amdgcn_wave_barrier();
            // ---- Cholesky, column by column; every element's own k-sum runs k = 0..j-1
            for (int j = 0; j < OM_D && ok; ++j) {
                if (lane == j) {
                    double r = B[j * OM_LD + j];
                    for (int k = 0; k < j; ++k) r = r - L[j * OM_LD + k] * L[j * OM_LD + k];
                    L[j * OM_LD + j] = r > 0.0 && isfinite(r) ? sqrt(r) : -1.0;
                }
                __builtin_amdgcn_wave_barrier();
                const double ljj = L[j * OM_LD + j];
                ok = ljj > 0.0;                                // (a pivot that is not > 0 or not finite left -1 here)
                if (ok && lane > j && lane < OM_D) {
                    double r = B[lane * OM_LD + j];
                    for (int k = 0; k < j; ++k) r = r - L[lane * OM_LD + k] * L[j * OM_LD + k];
                    L[lane * OM_LD + j] = r / ljj;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (ok) {
            // ---- A = L^-1: lane j solves column j, rows j..15 in order, each k-sum k = j..i-1 from 0
            if (lane < OM_D) {
                const int j = lane;
                Ai[j * OM_LD + j] = 1.0 / L[j * OM_LD + j];
                for (int i2 = j + 1; i2 < OM_D; ++i2) {
                    double r = 0.0;
                    for (int k = j; k < i2; ++k) r = r - L[i2 * OM_LD + k] * Ai[k * OM_LD + j];
                    Ai[i2 * OM_LD + j] = r / L[i2 * OM_LD + i2];
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    float out[4];
    bool fin = true;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = lane + 64 * u, r = e >> 4, q = e & 15;
        out[u] = ok && q <= r ? (float)Ai[r * OM_LD + q] : 0.f;
        fin = fin && isfinite(out[u]);
    }
    ok = ok && __ballot(!fin) == 0ull;                         // a factor that leaves f32 is no metric either
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = lane + 64 * u, r = e >> 4, q = e & 15;
        a.A[(size_t)t * OM_D * OM_D + e] = ok ? out[u] : (r == q ? 1.f : 0.f);
    }
    if (lane == 0) a.valid[t] = ok ? 1 : 0;
}

// the transform of one window: y = A e over the lower triangle (f32, j ascending, from 0), then y / |y| as ol_tail_run forms
// z / |z|.  A: 256 floats in LDS, row-major.
__device__ __forceinline__ void om_transform(const float* A, float (&e)[OM_D]) {
#pragma clang fp contract(off)
    float y[OM_D], ss = 0.f;
#pragma unroll
    for (int i = 0; i < OM_D; ++i) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j <= i; ++j) s += A[i * OM_D + j] * e[j];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < OM_D; ++i) ss += y[i] * y[i];
    const float nrm = sqrtf(ss);
#pragma unroll
    for (int i = 0; i < OM_D; ++i) e[i] = y[i] / nrm;
}

constexpr int OM_APPLY_THREADS = 256;

__global__ __launch_bounds__(OM_APPLY_THREADS) void om_apply_kernel(const float* __restrict__ emb, long long n_rows,
                                                                    const float* __restrict__ A, float* __restrict__ out) {
    __shared__ float As[OM_D * OM_D];
    As[threadIdx.x] = A[threadIdx.x];
    __syncthreads();
    const long long w = (long long)blockIdx.x * OM_APPLY_THREADS + threadIdx.x;
    if (w >= n_rows) return;
    float e[OM_D];
    const float4* src = (const float4*)(emb + (size_t)w * OM_D);
#pragma unroll
    for (int q = 0; q < OM_D / 4; ++q) {
        const float4 v = src[q];
        e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w;
    }
    om_transform(As, e);
    float4* dst = (float4*)(out + (size_t)w * OM_D);
#pragma unroll
    for (int q = 0; q < OM_D / 4; ++q) dst[q] = make_float4(e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the stage: embeddings -> whitened unit embeddings -> logits against the user's rows, prediction, vote
// ---------------------------------------------------------------------------------------------------------------------------
// Per-stream state.  A zeroed state is a valid start: no metric, no classes, empty ring.
struct OmState {
    int K;                               // class rows
    int has_metric;
    int head, len;                       // ring position and fill
    int ids[OM_MAXK];                    // class id of each slot, ascending
    int ring[OL_MAXVOTE];                // slot of each window's prediction, -1: none
    float A[OM_D * OM_D];                // the metric, lower triangular, row-major
    float row[OM_MAXK][OM_D];            // the unit class rows of the whitened space
};

struct OmPushArgs {
    OmState* states;
    const float* emb;                    // [total_rows][16]
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int total_rows, ldl, vote;
    int32_t* pred;                       // [total_rows] class id or -1
    int32_t* voted;                      // [total_rows] class id or -1
    float* logits;                       // optional [total_rows][ldl]
};

__global__ __launch_bounds__(64) void om_push_kernel(OmPushArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float es[OM_MAXM * OM_D];
    __shared__ float As[OM_D * OM_D];
    __shared__ int ring[OL_MAXVOTE];
    __shared__ int row_pred[OM_MAXM], row_voted[OM_MAXM];
    OmState* st = a.states + blockIdx.x;
    const int lane = threadIdx.x;
    const int K = st->K, M = a.m[blockIdx.x], r0 = a.row0[blockIdx.x], V = a.vote;
    // a stream without a metric or without rows, or whose rows disagree with the limits, is left untouched
    if (K < 1 || K > OM_MAXK || st->has_metric != 1 || M < 1 || M > OM_MAXM || r0 < 0 || r0 > a.total_rows - M) return;
    if (a.logits && K > a.ldl) return;
    const bool on = lane < K;
    const int my_id = on ? st->ids[lane] : -1;
    float row[OM_D];
#pragma unroll
    for (int q = 0; q < OM_D / 4; ++q) {
        const float4 v = on ? *(const float4*)(st->row[lane] + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        row[4 * q] = v.x; row[4 * q + 1] = v.y; row[4 * q + 2] = v.z; row[4 * q + 3] = v.w;
    }
    for (int i = lane; i < OM_D * OM_D; i += 64) As[i] = st->A[i];
    int head = st->head, len = st->len;
    if (head < 0 || head >= V || len < 0 || len > V) {         // a ring kept under another vote length: start empty
        head = 0;
        len = 0;
    }
    for (int i = lane; i < V; i += 64) ring[i] = st->ring[i];
    const float4* src = (const float4*)(a.emb + (size_t)r0 * OM_D);
    for (int i = lane; i < M * (OM_D / 4); i += 64) ((float4*)es)[i] = src[i];
    __builtin_amdgcn_wave_barrier();
    int cnt = 0;                                               // entries of slot `lane` in the ring
    for (int i = 0; i < len; ++i) cnt += ring[(head + V - len + i) % V] == lane;
    for (int w = lane; w < M; w += 64) {                       // the transform, one window per lane, in place
        float e[OM_D];
#pragma unroll
        for (int q = 0; q < OM_D / 4; ++q) {
            const float4 v = ((const float4*)es)[w * (OM_D / 4) + q];
            e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w;
        }
        om_transform(As, e);
#pragma unroll
        for (int q = 0; q < OM_D / 4; ++q) ((float4*)es)[w * (OM_D / 4) + q] = make_float4(e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]);
    }
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < M; ++j) {
        float ev[OM_D];
#pragma unroll
        for (int q = 0; q < OM_D / 4; ++q) {
            const float4 v = *(const float4*)(es + j * OM_D + 4 * q);
            ev[4 * q] = v.x; ev[4 * q + 1] = v.y; ev[4 * q + 2] = v.z; ev[4 * q + 3] = v.w;
        }
        float l = 0.f;
#pragma unroll
        for (int d = 0; d < OM_D; ++d) l += ev[d] * row[d];
        if (a.logits && on) a.logits[(size_t)(r0 + j) * a.ldl + lane] = l;
        const bool bad = __ballot(on && !isfinite(l)) != 0ull;
        int k1 = -1;                                           // a window with a logit that is not finite predicts nothing
        if (!bad) k1 = 255 - (int)(ot_wave_max(ot_key(on, l, lane)) & 255u);
        int vj = ol_vote_step(ring, head, len, cnt, V, k1, lane);
        if (__shfl(cnt, vj, 64) == 0) vj = -1;                 // no slot has an entry
        const int pid = __shfl(my_id, max(k1, 0), 64), vid = __shfl(my_id, max(vj, 0), 64);
        if (lane == 0) {
            row_pred[j] = k1 >= 0 ? pid : -1;
            row_voted[j] = vj >= 0 ? vid : -1;
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int j = lane; j < M; j += 64) {
        a.pred[r0 + j] = row_pred[j];
        a.voted[r0 + j] = row_voted[j];
    }
    for (int i = lane; i < V; i += 64) st->ring[i] = ring[i];
    if (lane == 0) {
        st->head = head;
        st->len = len;
    }
}

struct OmIds {
    int ids[OM_MAXK];
    int K;
};

// installs the metric (A: 256 floats, the strict upper triangle is not read) and / or the class rows (rows / |row| as
// ol_set_classes_kernel forms them, and their ids); what is NULL stays.  The ring empties.
__global__ __launch_bounds__(64) void om_set_kernel(OmState* st, const float* __restrict__ A, const float* __restrict__ rows, OmIds c) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    if (A) {
        for (int e = lane; e < OM_D * OM_D; e += 64) st->A[e] = (e & 15) <= (e >> 4) ? A[e] : 0.f;
    }
    if (rows) {
        const bool on = lane < c.K;
        float ss = 0.f;
        if (on)
            for (int d = 0; d < OM_D; ++d) ss += rows[lane * OM_D + d] * rows[lane * OM_D + d];
        const float n = sqrtf(ss);
        for (int d = 0; d < OM_D; ++d) st->row[lane][d] = on ? rows[lane * OM_D + d] / n : 0.f;
        st->ids[lane] = on ? c.ids[lane] : -1;
    }
    if (lane == 0) {
        if (A) st->has_metric = 1;
        if (rows) st->K = c.K;
        st->head = 0;
        st->len = 0;
    }
}

// streams first .. first + gridDim.x - 1: the ring to empty; what != 0: the metric and the rows leave as well
__global__ __launch_bounds__(64) void om_reset_kernel(OmState* states, int first, int what) {
    OmState* st = states + first + blockIdx.x;
    if (threadIdx.x == 0) {
        st->head = 0;
        st->len = 0;
        if (what) {
            st->K = 0;
            st->has_metric = 0;
        }
    }
}
