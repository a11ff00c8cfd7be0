// Held-out enrolment scoring (include/cpnative.h, cp_online_holdout_*): leave-a-repetition-out over one cued recording's
// embeddings.  A plan names the repetitions that train the class rows (a bit mask), the repetitions that are scored (a bit
// mask), and the mix and min_windows of the enrolment.  holdout_reference of contrastiveprosthetics_amd/holdout.py is the
// definition; the device equals it in every integer and bit.
//
//   oh_sums_kernel    one thread per (training mask u, slot c, dimension d): a wave is four masks x sixteen dimensions of one
//                     slot, so the slot test is uniform over the wave and a window's 64-byte embedding row is one coalesced
//                     load.  The wave takes 64 windows at a time, finds those of its slot with one ballot and walks them in
//                     window order: every (u, c, d) sum is one float64 add per training window in window order, which is the
//                     accumulator cp_online_enroll leaves.  No atomics, nothing is reduced across lanes.
//   oh_tables_kernel  one thread per (plan, slot): the blend of ole_table_kernel with the plan's mix and min_windows, then the
//                     unit row as ol_set_classes_kernel forms it.
//   oh_score_kernel   one wave per plan, one wave per workgroup; lane k holds class k's unit row in registers.  Windows come 64
//                     at a time (slot and repetition one per lane, the evaluated embeddings through LDS); the evaluated ones
//                     are walked in order: every lane's logit, the first maximum as a wave maximum of (value, 255 - lane) keys
//                     (ot_key), the decoders' vote ring (ol_vote_step), the counters.  With CONF the two confusion tables
//                     live in LDS, cell (cue, predicted) owned by lane `predicted`.  The training windows are only counted.
//   oh_logits_kernel  row-parallel: window i against the unit rows of plan assign[i], NaN where there is none.
// Every value read from the device is checked before it is an index: a slot outside 0..K-1, a repetition outside 0..31, a
// plan's sums index, an assignment outside 0..n_plans-1.
#pragma once
#include "online_enroll.cuh"
#include "online_subsets.cuh"
#include "online_track.cuh"

constexpr int OH_MAXK = 64;              // class slots (CP_ONLINE_MAX_CLASSES): one per lane
constexpr int OH_D = 16;                 // embedding width (CP_D_E)
constexpr int OH_SCORES = 9;             // CP_ONLINE_HOLDOUT_SCORES, in the order of HOLDOUT_SCORE_KEYS
constexpr int OH_MAX_PLANS = 4096;       // CP_ONLINE_HOLDOUT_MAX_PLANS
constexpr int OH_MAX_REPS = 32;          // CP_ONLINE_HOLDOUT_MAX_REPS: the bits of a mask
constexpr int OH_NOT_EVALUATED = -3;     // a sequence entry of a window the plan does not score
constexpr int OH_SUM_MASKS = 4;          // training masks per wave of oh_sums_kernel

struct OhPlan {                          // cp_online_holdout_plan, on the device: checked by the kernels
    uint32_t train, eval;
    int32_t sums_index, min_windows;
    double mix;
};

// a plan the definition refuses: nothing is indexed with it
__device__ __forceinline__ bool oh_plan_ok(const OhPlan& p, int n_masks) {
    return p.mix >= 0.0 && p.mix <= 1.0 && p.min_windows >= 1 && p.sums_index >= 0 && p.sums_index < n_masks;
}

// grid (ceil(n_masks / 4), 64), 64 threads: sums[u][c][0..15] and the count sums[u][c][16] of slot c = blockIdx.y
__global__ __launch_bounds__(64) void oh_sums_kernel(const float* __restrict__ emb, long long n_rows, int K,
                                                     const int32_t* __restrict__ slot, const int32_t* __restrict__ rep,
                                                     const uint32_t* __restrict__ masks, int n_masks, double* __restrict__ sums) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, d = lane & 15, c = blockIdx.y;
    const int u = blockIdx.x * OH_SUM_MASKS + (lane >> 4);
    const bool have = u < n_masks;
    const uint32_t mask = have ? masks[u] : 0u;
    double sum = 0.0;
    long long cnt = 0;
    if (c < K) {                                               // (uniform over the wave)
        for (long long base = 0; base < n_rows; base += 64) {
            int s = -1, r = -1;
            if (base + lane < n_rows) {
                s = slot[base + lane];
                r = rep[base + lane];
            }
            unsigned long long todo = __ballot(s == c && r >= 0 && r < OH_MAX_REPS);
            while (todo) {                                     // the slot's windows of this block in window order
                const int j = og_first(todo);
                todo &= todo - 1ull;
                const int rj = __builtin_amdgcn_readlane(r, j);
                const float e = emb[(size_t)(base + j) * OH_D + d];
                if ((mask >> rj) & 1u) {
                    sum += (double)e;
                    ++cnt;
                }
            }
        }
    }
    if (have) {
        double* out = sums + ((size_t)u * OH_MAXK + c) * OLE_ACC_W;
        out[d] = sum;
        if (d == 0) out[16] = (double)cnt;
    }
}

// grid n_plans, 64 threads: thread c blends slot c of the plan as ole_table_kernel does and normalises as
// ol_set_classes_kernel does
__global__ __launch_bounds__(64) void oh_tables_kernel(const double* __restrict__ sums, int n_masks, int K,
                                                       const float* __restrict__ prior, const OhPlan* __restrict__ plans,
                                                       float* __restrict__ rows, float* __restrict__ unit) {
#pragma clang fp contract(off)
    const int c = threadIdx.x, t = blockIdx.x;
    const OhPlan p = plans[t];
    if (c >= K || !oh_plan_ok(p, n_masks)) return;
    const double* acc = sums + ((size_t)p.sums_index * OH_MAXK + c) * OLE_ACC_W;
    const double mix = p.mix, min_windows = (double)p.min_windows;
    float ss = 0.f;
    for (int d = 0; d < OH_D; ++d) ss += prior[c * OH_D + d] * prior[c * OH_D + d];
    const double len = (double)sqrtf(ss);
    double s2 = 0.0;
    for (int d = 0; d < OH_D; ++d) s2 += acc[d] * acc[d];
    const double sn = sqrt(s2);
    const bool enrolled = acc[16] >= min_windows && sn > 0.0;
    float row[OH_D], rs = 0.f;
#pragma unroll
    for (int d = 0; d < OH_D; ++d) {
        const float e = prior[c * OH_D + d];
        float v = e;
        if (enrolled) {
            const double q = acc[d] / sn;
            v = len > 0.0 ? (float)((1.0 - mix) * (double)e + mix * (len * q)) : (float)q;
        }
        row[d] = v;
    }
#pragma unroll
    for (int d = 0; d < OH_D; ++d) rs += row[d] * row[d];
    const float n = sqrtf(rs);
    const size_t at = ((size_t)t * K + c) * OH_D;
#pragma unroll
    for (int d = 0; d < OH_D; ++d) {
        rows[at + d] = row[d];
        unit[at + d] = row[d] / n;
    }
}

struct OhScoreArgs {
    const float* emb;                    // [n_rows][16]
    const int32_t* slot;                 // [n_rows] slot, -1 rest; anything else: not scored and never trained
    const int32_t* rep;                  // [n_rows] repetition 0..31; anything else: neither trained nor evaluated
    const float* unit;                   // [n_plans][K][16]
    const OhPlan* plans;                 // [n_plans], on the device: not checked by the host
    long long n_rows;
    int n_plans, K, vote;
    long long* scores;                   // [n_plans][OH_SCORES]
    int32_t* confusion;                  // optional [n_plans][64][64]
    int32_t* voted_confusion;            // optional
    int32_t* pred;                       // optional [n_plans][n_rows] slot, -1 none, -3 not evaluated
    int32_t* voted;                      // optional
};

template <bool CONF>
__global__ __launch_bounds__(64) void oh_score_kernel(OhScoreArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float es[64 * OH_D];
    __shared__ int ring[OL_MAXVOTE];
    __shared__ int hist[OH_MAXK];
    __shared__ int conf[CONF ? 2 * OH_MAXK * OH_MAXK : 1];         // [cue][predicted], then [cue][voted]
    constexpr int VC = OH_MAXK * OH_MAXK;                          // where the voted table starts
    const int lane = threadIdx.x, t = blockIdx.x;
    const OhPlan p = a.plans[t];
    long long* out = a.scores + (size_t)t * OH_SCORES;
    if (!oh_plan_ok(p, OH_MAX_PLANS)) {
        if (lane < OH_SCORES) out[lane] = -1;                  // a plan the definition refuses: nothing else is written
        return;
    }
    const int K = a.K, V = a.vote;
    const bool on = lane < K;
    float row[OH_D];
#pragma unroll
    for (int q = 0; q < OH_D / 4; ++q) {
        const float4 v = on ? *(const float4*)(a.unit + ((size_t)t * K + lane) * OH_D + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        row[4 * q] = v.x; row[4 * q + 1] = v.y; row[4 * q + 2] = v.z; row[4 * q + 3] = v.w;
    }
    if constexpr (CONF) {
        for (int i = lane; i < 2 * VC; i += 64) conf[i] = 0;
    }
    int head = 0, len = 0, cnt = 0;                            // the ring; cnt: entries of slot `lane` in it
    long long n_train_c = 0;                                   // training windows of slot `lane`
    int class_n = 0, class_hit = 0;                            // cue rows of class `lane`, and those whose vote is that class
    long long n_cue = 0, pred_hit = 0, voted_hit = 0, n_rest = 0;
    for (long long base = 0; base < a.n_rows; base += 64) {
        const int nb = (int)min((long long)64, a.n_rows - base);
        int s = -2, r = -1;
        if (lane < nb) {
            s = a.slot[base + lane];
            r = a.rep[base + lane];
            if (s < -1 || s >= K) s = -2;                      // not scored, never trained
            if (r < 0 || r >= OH_MAX_REPS) r = -1;
        }
        const bool trains = r >= 0 && s >= 0 && ((p.train >> r) & 1u) != 0u;
        const bool evals = r >= 0 && ((p.eval >> r) & 1u) != 0u;
        __builtin_amdgcn_wave_barrier();                       // (one wave: the block before has read es and hist)
        hist[lane] = 0;
        if (evals) {
            const float4* src = (const float4*)(a.emb + (size_t)(base + lane) * OH_D);
#pragma unroll
            for (int q = 0; q < OH_D / 4; ++q) ((float4*)es)[lane * (OH_D / 4) + q] = src[q];
        }
        __builtin_amdgcn_wave_barrier();
        if (trains) atomicAdd(&hist[s], 1);                    // (an integer count in LDS: the order does not matter)
        __builtin_amdgcn_wave_barrier();
        n_train_c += hist[lane];
        int my_pred = OH_NOT_EVALUATED, my_voted = OH_NOT_EVALUATED;
        unsigned long long todo = __ballot(evals);
        while (todo) {                                         // the evaluated windows of this block in window order
            const int j = og_first(todo);
            todo &= todo - 1ull;
            float ev[OH_D];
#pragma unroll
            for (int q = 0; q < OH_D / 4; ++q) {
                const float4 v = *(const float4*)(es + j * OH_D + 4 * q);
                ev[4 * q] = v.x; ev[4 * q + 1] = v.y; ev[4 * q + 2] = v.z; ev[4 * q + 3] = v.w;
            }
            float l = 0.f;
#pragma unroll
            for (int d = 0; d < OH_D; ++d) l += ev[d] * row[d];
            const bool bad = __ballot(on && !isfinite(l)) != 0ull;
            int k1 = -1;                                       // a row with a logit that is not finite predicts nothing
            if (!bad) k1 = 255 - (int)(ot_wave_max(ot_key(on, l, lane)) & 255u);
            int vj = ol_vote_step(ring, head, len, cnt, V, k1, lane);
            if (__shfl(cnt, vj, 64) == 0) vj = -1;             // no slot has an entry
            if (lane == j) {
                my_pred = k1;
                my_voted = vj;
            }
            const int ej = __builtin_amdgcn_readlane(s, j);
            n_rest += ej == -1;
            if (ej >= 0) {
                ++n_cue;
                pred_hit += k1 == ej;
                voted_hit += vj == ej;
                if (lane == ej) {
                    ++class_n;
                    class_hit += vj == ej;
                }
                if constexpr (CONF) {
                    if (lane == k1) ++conf[ej * OH_MAXK + lane];
                    if (lane == vj) ++conf[VC + ej * OH_MAXK + lane];
                }
            }
        }
        if (lane < nb) {
            const size_t at = (size_t)t * a.n_rows + base + lane;
            if (a.pred) a.pred[at] = my_pred;
            if (a.voted) a.voted[at] = my_voted;
        }
    }
    // ---- the counters of the training side
    long long n_train = n_train_c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_train += __shfl_xor(n_train, o, 64);
    const long long n_enrolled = __popcll(__ballot(on && n_train_c >= (long long)p.min_windows));
    // ---- the class with the smallest voted recall class_hit / class_n, the smallest slot among equals
    unsigned long long have = __ballot(class_n > 0);
    long long worst = -1, worst_hit = 0, worst_n = 0;
    while (have) {
        const int k = og_first(have);
        have &= have - 1ull;
        const long long h = __builtin_amdgcn_readlane(class_hit, k), n = __builtin_amdgcn_readlane(class_n, k);
        if (worst < 0 || h * worst_n < worst_hit * n) {
            worst = k;
            worst_hit = h;
            worst_n = n;
        }
    }
    const long long sc[OH_SCORES] = {n_cue, pred_hit, voted_hit, n_rest, n_train, n_enrolled, worst, worst_hit, worst_n};
#pragma unroll
    for (int i = 0; i < OH_SCORES; ++i)
        if (lane == i) out[i] = sc[i];
    if constexpr (CONF) {
        __builtin_amdgcn_wave_barrier();
        const size_t at = (size_t)t * VC;
        for (int i = lane; i < VC; i += 64) {
            if (a.confusion) a.confusion[at + i] = conf[i];
            if (a.voted_confusion) a.voted_confusion[at + i] = conf[VC + i];
        }
    }
}

// grid ceil(n_rows / 4), 256 threads: one wave per window, lane k = slot k
__global__ __launch_bounds__(256) void oh_logits_kernel(const float* __restrict__ emb, long long n_rows, int K,
                                                        const float* __restrict__ unit, int n_plans,
                                                        const int32_t* __restrict__ assign, float* __restrict__ logits, int ldl) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_rows || lane >= K) return;
    const int t = assign[i];
    float l = __int_as_float(0x7FC00000);                      // no plan: NaN
    if (t >= 0 && t < n_plans) {
        const float* e = emb + (size_t)i * OH_D;
        const float* u = unit + ((size_t)t * K + lane) * OH_D;
        l = 0.f;
#pragma unroll
        for (int d = 0; d < OH_D; ++d) l += e[d] * u[d];
    }
    logits[(size_t)i * ldl + lane] = l;
}
