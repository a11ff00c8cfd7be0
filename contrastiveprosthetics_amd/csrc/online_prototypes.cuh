// Posture prototypes (include/cpnative.h, cp_online_proto_fit and cp_online_group_*): several class rows per grasp.  A grasp made
// in different arm positions lands in different places of the 16-d space; the fit finds up to four rows per class from a cued
// recording's embeddings (farthest-first seeding, then Lloyd rounds on the sphere), and the group stage turns the row logits
// of a decoder that holds such a table back into class logits, a class prediction and a class vote.  fit_reference and
// group_reference of contrastiveprosthetics_amd/prototypes.py are the definitions; the device equals them in every integer and
// bit.
//
//   op_fit_kernel       grid n_classes + 1, one wave each; the whole fit of one class is one wave's work, so nothing is reduced
//                       across workgroups and a class's result cannot depend on the other classes.  The windows come 64 at a
//                       time, one per lane: the lane tests its window (slot, use, all 16 components finite), keeps its 16 floats
//                       in registers and forms its own dot products against the centres, which lie in LDS (every lane reads the
//                       same address: a broadcast).  The sums need window order, so the block's rows also go through LDS and the
//                       class's windows, found by one ballot, are walked in order with lane = (centre, dimension): lane
//                       (winner, d) makes the one float64 add.  Farthest-first is a wave maximum of (value, window index) keys,
//                       each lane keeping the maximum of its own windows first: the result does not depend on how windows are
//                       dealt to lanes.  The last workgroup writes assign = -1 for the windows of no class.
//   opg_push_kernel     grid n_streams, one wave each, the stage form of og_push_kernel: lane r holds row slot r, lane g group
//                       slot g and the 64-bit mask of its rows.  Four windows' logits go through LDS at a time; lane g takes the
//                       first maximum of its rows, the prediction is a wave maximum of (value, 255 - lane) keys (ot_key), the
//                       vote the decoders' ring (ol_vote_step).
//   opg_set_groups_kernel, opg_reset_kernel   one wave per stream.
// Everything is integer, single f32 or single f64 operations with floating-point contraction off and no atomics.  Every value
// read from the device is checked before it is an index: a slot outside 0..K-1 belongs to no class, the winner of a
// farthest-first round is tested against n_rows, a stream's row0 / m / R / G against the limits; ring entries and group slots
// are only ever compared with a lane.
#pragma once
#include "online_holdout.cuh"

constexpr int OP_MAXK = 64;              // class slots (CP_ONLINE_MAX_CLASSES)
constexpr int OP_D = 16;                 // embedding width (CP_D_E)
constexpr int OP_MAXR = 4;               // rows per class (CP_ONLINE_PROTO_MAX_ROWS): 4 centres x 16 dimensions = one wave
constexpr int OP_MAX_ITERS = 64;         // CP_ONLINE_PROTO_MAX_ITERS

struct OpFitArgs {
    const float* emb;                    // [n_rows][16]
    const int32_t* slot;                 // [n_rows] class slot; anything outside 0..K-1: the window belongs to no class
    const uint8_t* use;                  // optional [n_rows]: 0: the window does not train
    long long n_rows;
    int K, iters, min_windows;
    unsigned char rows_per_class[OP_MAXK];       // 1..4, checked on the host
    float* rows;                         // [K][4][16]
    long long* counts;                   // [K][4]
    uint8_t* valid;                      // [K][4]
    long long* moved;                    // [K][iters]
    int32_t* assign;                     // [n_rows] row index within the class, -1: the window did not train
};

// a float as an integer that orders as the float does; -0 counts as +0 (the mapping of ot_key)
__device__ __forceinline__ unsigned op_ordered(float v) {
    const unsigned u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// what a lane knows of its window of the block at `base`
struct OpWin {
    float e[OP_D];
    bool mine;                           // of class c, allowed to train, all 16 components finite
    bool of_class;                       // slot == c
};

__device__ __forceinline__ OpWin op_load(const OpFitArgs& a, int c, long long base, int lane) {
    OpWin w;
    const long long i = base + lane;
    int s = -1;
    bool u = false;
    if (i < a.n_rows) {
        s = a.slot[i];
        u = a.use ? a.use[i] != 0 : true;
    }
    w.of_class = s == c;
    bool fin = true;
#pragma unroll
    for (int d = 0; d < OP_D; ++d) w.e[d] = 0.f;
    if (w.of_class && u) {
        const float4* src = (const float4*)(a.emb + (size_t)i * OP_D);
#pragma unroll
        for (int q = 0; q < OP_D / 4; ++q) {
            const float4 v = src[q];
            w.e[4 * q] = v.x; w.e[4 * q + 1] = v.y; w.e[4 * q + 2] = v.z; w.e[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int d = 0; d < OP_D; ++d) fin = fin && isfinite(w.e[d]);
    }
    w.mine = w.of_class && u && fin;
    return w;
}

// the f32 dot product of the lane's window with one centre in LDS: products and sums rounded one by one, d ascending, from 0
__device__ __forceinline__ float op_dot(const float (&e)[OP_D], const float* cen) {
#pragma clang fp contract(off)
    float l = 0.f;
#pragma unroll
    for (int d = 0; d < OP_D; ++d) l += e[d] * cen[d];
    return l;
}

// One pass over the class's windows: every window goes to the centre with the largest dot product among the first Rn (the first
// maximum under `>`), and lane (centre, d) adds it to its float64 sum in window order.  store: the assignment is written, and
// -1 for the class's windows that do not train; track: windows whose assignment differs from the stored one are counted
// (first: all of them).  Returns that count (the same on every lane); sum and cnt are those of lane (q, d).
__device__ __forceinline__ long long op_walk(const OpFitArgs& a, int c, int lane, int Rn, bool store, bool track, bool first,
                                             const float* cen, float* es, double& sum, long long& cnt) {
#pragma clang fp contract(off)
    const int q = lane >> 4, d = lane & 15;
    sum = 0.0;
    cnt = 0;
    long long moved = 0;
    for (long long base = 0; base < a.n_rows; base += 64) {
        const OpWin w = op_load(a, c, base, lane);
        __builtin_amdgcn_wave_barrier();                       // (one wave: the block before has read es)
        if (w.mine) {
#pragma unroll
            for (int p = 0; p < OP_D / 4; ++p)
                ((float4*)es)[lane * (OP_D / 4) + p] = make_float4(w.e[4 * p], w.e[4 * p + 1], w.e[4 * p + 2], w.e[4 * p + 3]);
        }
        int best = 0;
        if (w.mine && Rn > 1) {
            float bv = op_dot(w.e, cen);
            for (int r = 1; r < Rn; ++r) {
                const float v = op_dot(w.e, cen + r * OP_D);
                if (v > bv) {
                    bv = v;
                    best = r;
                }
            }
        }
        bool differs = false;
        if (w.mine && track) differs = first || a.assign[base + lane] != best;
        moved += __popcll(__ballot(differs));
        if (store) {
            if (w.mine) a.assign[base + lane] = best;
            else if (w.of_class) a.assign[base + lane] = -1;
        }
        __builtin_amdgcn_wave_barrier();
        unsigned long long todo = __ballot(w.mine);
        while (todo) {                                         // the class's windows of this block in window order
            const int j = og_first(todo);
            todo &= todo - 1ull;
            const int aj = __builtin_amdgcn_readlane(best, j);
            if (q == aj) {
                sum += (double)es[j * OP_D + d];
                ++cnt;
            }
        }
    }
    return moved;
}

// centre q = (float)(S_q / |S_q|) where its count and |S_q| are > 0, |S_q| the float64 root of the squares summed with d
// ascending; otherwise it stays.  Returns |S_q| of the lane's centre.
__device__ __forceinline__ double op_update(int lane, int Rn, double sum, long long cnt, float* cen, double* sacc) {
#pragma clang fp contract(off)
    const int q = lane >> 4;
    __builtin_amdgcn_wave_barrier();
    sacc[lane] = sum;
    __builtin_amdgcn_wave_barrier();
    double s2 = 0.0;
#pragma unroll
    for (int d = 0; d < OP_D; ++d) s2 += sacc[q * OP_D + d] * sacc[q * OP_D + d];
    const double sn = sqrt(s2);
    if (q < Rn && cnt > 0 && sn > 0.0) cen[lane] = (float)(sum / sn);
    __builtin_amdgcn_wave_barrier();
    return sn;
}

// grid K + 1, 64 threads: workgroup c < K fits class slot c, workgroup K marks the windows of no class
__global__ __launch_bounds__(64) void op_fit_kernel(OpFitArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float es[64 * OP_D];
    __shared__ float cen[OP_MAXR * OP_D];
    __shared__ double sacc[64];
    const int lane = threadIdx.x, c = blockIdx.x, q = lane >> 4;
    const int K = a.K;
    if (c >= K) {
        for (long long i = lane; i < a.n_rows; i += 64) {
            const int s = a.slot[i];
            if (s < 0 || s >= K) a.assign[i] = -1;
        }
        return;
    }
    int R = a.rows_per_class[c];
    R = R < 1 ? 1 : (R > OP_MAXR ? OP_MAXR : R);
    cen[lane] = 0.f;
    long long my_moved = 0;                                    // lane t: moved[c][t]
    double sum;
    long long cnt;
    // ---- centre 0: the unit vector of the float64 sum of all the class's windows
    op_walk(a, c, lane, 1, false, false, false, cen, es, sum, cnt);
    const double sn0 = __shfl(op_update(lane, 1, sum, cnt, cen, sacc), 0, 64);
    const long long n0 = __shfl(cnt, 0, 64);
    const bool fitted = n0 >= (long long)a.min_windows && sn0 > 0.0;
    if (fitted) {                                              // (uniform over the wave)
        // ---- centres 1..R-1: the window farthest from the centres chosen so far, the earliest among equals
        for (int t = 1; t < R; ++t) {
            unsigned long long key = 0ull;
            for (long long base = 0; base < a.n_rows; base += 64) {
                const OpWin w = op_load(a, c, base, lane);
                if (w.mine) {
                    float nr = -INFINITY;
                    for (int r = 0; r < t; ++r) {
                        const float v = op_dot(w.e, cen + r * OP_D);
                        if (v > nr) nr = v;
                    }
                    const unsigned long long k2 = ((unsigned long long)(~op_ordered(nr)) << 32) | (0xFFFFFFFFu - (unsigned)(base + lane));
                    key = k2 > key ? k2 : key;
                }
            }
            key = ot_wave_max(key);
            const long long win = (long long)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
            __builtin_amdgcn_wave_barrier();
            if (key != 0ull && win < a.n_rows && lane < OP_D) cen[t * OP_D + lane] = a.emb[(size_t)win * OP_D + lane];
            __builtin_amdgcn_wave_barrier();
        }
        // ---- Lloyd rounds; once a round moves no window the centres are a fixed point and the rounds left would repeat it
        bool still = false;
        for (int t = 0; t < a.iters && !still; ++t) {
            const long long mv = op_walk(a, c, lane, R, true, true, t == 0, cen, es, sum, cnt);
            op_update(lane, R, sum, cnt, cen, sacc);
            if (lane == t) my_moved = mv;
            still = mv == 0;
        }
        // ---- the final assignment against the final centres
        op_walk(a, c, lane, R, true, false, false, cen, es, sum, cnt);
    } else {
        for (long long i = lane; i < a.n_rows; i += 64)
            if (a.slot[i] == c) a.assign[i] = -1;
        cnt = 0;
    }
    const bool have = fitted && q < R;
    a.rows[(size_t)c * OP_MAXR * OP_D + lane] = have ? cen[lane] : 0.f;
    if ((lane & 15) == 0) {
        a.counts[c * OP_MAXR + q] = have ? cnt : 0;
        a.valid[c * OP_MAXR + q] = have && cnt >= (long long)a.min_windows ? 1 : 0;
    }
    if (lane < a.iters) a.moved[(size_t)c * a.iters + lane] = my_moved;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the group stage: row logits -> class logits, class prediction, class vote
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int OPG_MAXM = 256;            // rows of one stream per push (CP_ONLINE_MAX_WINDOWS)

// Per-stream state.  A zeroed state is a valid start: no rows, no groups, empty ring.
struct OpgState {
    int R, G;                            // table rows and groups (classes)
    int head, len;                       // ring position and fill
    int row_ids[OP_MAXK];                // id of each table row, ascending
    int group_of[OP_MAXK];               // group slot of each table row
    int group_ids[OP_MAXK];              // class id of each group slot, ascending
    int ring[OL_MAXVOTE];                // group slot of each window's prediction, -1: none
};

struct OpgGroups {
    int row_ids[OP_MAXK], group_of[OP_MAXK], group_ids[OP_MAXK];
    int R, G;
};

struct OpgPushArgs {
    OpgState* states;
    const float* logits;                 // [total_rows][ldl]
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int ldl, total_rows, vote, ldc;
    int32_t* pred;                       // [total_rows] class id or -1
    int32_t* voted;                      // [total_rows] class id or -1
    int32_t* row;                        // [total_rows] row id or -1
    float* class_logits;                 // optional [total_rows][ldc]
};

__global__ __launch_bounds__(64) void opg_push_kernel(OpgPushArgs a) {
#pragma clang fp contract(off)
    __shared__ int ring[OL_MAXVOTE];
    __shared__ float lg[4][OP_MAXK];
    __shared__ int row_pred[OPG_MAXM], row_voted[OPG_MAXM], row_row[OPG_MAXM];
    OpgState* st = a.states + blockIdx.x;
    const int lane = threadIdx.x;
    const int R = st->R, G = st->G, M = a.m[blockIdx.x], r0 = a.row0[blockIdx.x], V = a.vote;
    // a stream without groups, or whose rows disagree with the limits, is left untouched
    if (R < 1 || R > OP_MAXK || G < 1 || G > R || R > a.ldl || M < 1 || M > OPG_MAXM || r0 < 0 || r0 > a.total_rows - M) return;
    if (a.class_logits && G > a.ldc) return;
    const bool on = lane < R, gon = lane < G;
    const int my_row_id = on ? st->row_ids[lane] : -1;
    const int my_grp = on ? st->group_of[lane] : -1;
    const int my_gid = gon ? st->group_ids[lane] : -1;
    unsigned long long mask = 0ull;                            // lane g: the rows of group g
    for (int g = 0; g < G; ++g) {
        const unsigned long long b = __ballot(on && my_grp == g);
        if (lane == g) mask = b;
    }
    int head = st->head, len = st->len;
    if (head < 0 || head >= V || len < 0 || len > V) {         // a ring kept under another vote length: start empty
        head = 0;
        len = 0;
    }
    for (int i = lane; i < V; i += 64) ring[i] = st->ring[i];
    __builtin_amdgcn_wave_barrier();
    int cnt = 0;                                               // entries of group `lane` in the ring
    for (int i = 0; i < len; ++i) cnt += ring[(head + V - len + i) % V] == lane;
    for (int j0 = 0; j0 < M; j0 += 4) {
        float l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) l[u] = on && j0 + u < M ? a.logits[(size_t)(r0 + j0 + u) * a.ldl + lane] : 0.f;
        __builtin_amdgcn_wave_barrier();                       // (one wave: the four windows before have read lg)
#pragma unroll
        for (int u = 0; u < 4; ++u) lg[u][lane] = l[u];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u;
            if (j >= M) break;
            const bool bad = __ballot(on && !isfinite(l[u])) != 0ull;
            float best = -INFINITY;                            // the first maximum of the group's rows, in row order
            int br = -1;
            bool nan = false;
            unsigned long long todo = mask;
            while (todo) {
                const int r = og_first(todo);
                todo &= todo - 1ull;
                const float v = lg[u][r];
                nan = nan || v != v;
                if (br < 0 || v > best) {
                    best = v;
                    br = r;
                }
            }
            const float cl = nan ? __int_as_float(0x7FC00000) : best;
            if (a.class_logits && gon) a.class_logits[(size_t)(r0 + j) * a.ldc + lane] = cl;
            int k1 = -1;                                       // a window with a logit that is not finite predicts nothing
            if (!bad) {
                const unsigned long long key = ot_wave_max(ot_key(gon && br >= 0, cl, lane));
                if (key != 0ull) k1 = 255 - (int)(key & 255u);
            }
            const int wr = k1 >= 0 ? __shfl(br, k1, 64) : -1;
            int vj = ol_vote_step(ring, head, len, cnt, V, k1, lane);
            if (__shfl(cnt, vj, 64) == 0) vj = -1;             // no group has an entry
            const int pid = __shfl(my_gid, max(k1, 0), 64), vid = __shfl(my_gid, max(vj, 0), 64);
            const int rid = __shfl(my_row_id, max(wr, 0), 64);
            if (lane == 0) {
                row_pred[j] = k1 >= 0 ? pid : -1;
                row_voted[j] = vj >= 0 ? vid : -1;
                row_row[j] = wr >= 0 ? rid : -1;
            }
        }
    }
    __syncthreads();
    for (int j = lane; j < M; j += 64) {
        a.pred[r0 + j] = row_pred[j];
        a.voted[r0 + j] = row_voted[j];
        a.row[r0 + j] = row_row[j];
    }
    for (int i = lane; i < V; i += 64) st->ring[i] = ring[i];
    if (lane == 0) {
        st->head = head;
        st->len = len;
    }
}

// installs rows, groups and their ids; the ring empties
__global__ __launch_bounds__(64) void opg_set_groups_kernel(OpgState* st, OpgGroups g) {
    const int lane = threadIdx.x;
    st->row_ids[lane] = lane < g.R ? g.row_ids[lane] : -1;
    st->group_of[lane] = lane < g.R ? g.group_of[lane] : -1;
    st->group_ids[lane] = lane < g.G ? g.group_ids[lane] : -1;
    if (lane == 0) {
        st->R = g.R;
        st->G = g.G;
        st->head = 0;
        st->len = 0;
    }
}

// the ring of streams first .. first + gridDim.x - 1 to empty; rows and groups stay
__global__ __launch_bounds__(64) void opg_reset_kernel(OpgState* states, int first) {
    OpgState* st = states + first + blockIdx.x;
    if (threadIdx.x == 0) {
        st->head = 0;
        st->len = 0;
    }
}
