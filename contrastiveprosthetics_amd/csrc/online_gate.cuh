// Grasp command gate (include/cpnative.h, cp_online_gate_*): the logits of an online decoder -> a command a hand can follow.
// A stage behind the decoders: it reads the cosines their tails emit and keeps one state machine per stream in a workspace
// of its own (OgState), so the decoders' kernels and outputs stay as they are and one kernel serves all four of them.
//
//   og_push_kernel   grid n_streams, one wave each; lane k serves class slot k.  Pass 1 classifies the stream's rows four at
//                    a time (the rows do not depend on the state, so their loads are in flight together): first maximum,
//                    runner-up, margin, accept or reject, integer weight; slot and weight of every row go to LDS, accepted,
//                    conf and margin to the caller.  Pass 2 walks the rows in window order: the entry enters the ring, lane k
//                    keeps the count and the integer weight sum of slot k over the ring (sliding, exact), the candidate is a
//                    wave maximum, and the command / pending / run update is uniform over the wave.  The commands of the
//                    push leave LDS in one coalesced store.
//   og_set_classes_kernel, og_reset_kernel   one wave per stream.
// Everything is integer or single f32 operations with floating-point contraction off: the outputs are the same for any
// cutting of a stream's rows into calls and for any set of streams that share a launch.
#pragma once
#include "common.cuh"

constexpr int OG_MAXK = 64;              // class slots (CP_ONLINE_MAX_CLASSES): one per lane
constexpr int OG_MAXVOTE = 256;          // ring length (CP_ONLINE_MAX_VOTE)
constexpr int OG_MAXM = 256;             // rows of one stream per push (CP_ONLINE_MAX_WINDOWS)
constexpr float OG_WEIGHT_SCALE = 1048576.f;        // 2^20: margin <= 2 -> weight <= 2^21 + 1, 256 of them < 2^31

// Per-stream state.  A zeroed state is a valid start: no classes, empty ring, nothing pending, command none.
struct OgState {
    int K;                               // ---- class part (survives a reset)
    int head, len;                       // ---- stream part: ring position and fill
    int command;                         // class id + 1; 0: none
    int pending;                         // slot, or -1 for none; meaningful while run > 0
    int run;                             // windows the pending candidate has won in a row; 0: nothing pending
    int pad[2];
    int ids[OG_MAXK];                    // class id of each slot, ascending, >= 0
    float min_cosine[OG_MAXK];
    int ring_slot[OG_MAXVOTE];           // slot of the window's first maximum, or -1 (rejected)
    int ring_w[OG_MAXVOTE];              // its integer weight
};

struct OgConfig {                        // cp_online_gate_config, checked on the host
    int vote, min_votes, dwell, release, weight;
    float min_margin;
};

struct OgPushArgs {
    OgState* states;
    const float* logits;                 // [total_rows][ldl]
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int ldl, total_rows;
    int32_t* command;                    // [total_rows] class id or -1
    int32_t* accepted;                   // [total_rows] class id or -1
    float* conf;                         // optional [total_rows]
    float* margin;                       // optional [total_rows]
    OgConfig c;
};

__device__ __forceinline__ float og_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int og_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// first lane of a non-empty ballot
__device__ __forceinline__ int og_first(unsigned long long mask) { return __ffsll((long long)mask) - 1; }

__global__ __launch_bounds__(64) void og_push_kernel(OgPushArgs a) {
#pragma clang fp contract(off)
    __shared__ int ring_slot[OG_MAXVOTE], ring_w[OG_MAXVOTE];
    __shared__ int row_slot[OG_MAXM], row_w[OG_MAXM], row_cmd[OG_MAXM];
    OgState* st = a.states + blockIdx.x;
    const int lane = threadIdx.x;
    const int K = st->K, M = a.m[blockIdx.x], r0 = a.row0[blockIdx.x];
    // a stream without classes, or whose rows disagree with the limits, is left untouched
    if (K < 1 || K > OG_MAXK || K > a.ldl || M < 1 || M > OG_MAXM || r0 < 0 || r0 > a.total_rows - M) return;
    const bool on = lane < K;
    const int my_id = on ? st->ids[lane] : -1;
    const float my_thr = on ? st->min_cosine[lane] : 0.f;
    const float nan = __builtin_nanf("");

    // ---- pass 1: the rows on their own
    for (int j0 = 0; j0 < M; j0 += 4) {
        float l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            l[u] = on && j0 + u < M ? a.logits[(size_t)(r0 + j0 + u) * a.ldl + lane] : -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u;
            if (j >= M) break;
            const bool bad = __ballot(on && !isfinite(l[u])) != 0ull;
            const float c1 = og_wave_max(l[u]);
            const int k1 = og_first(__ballot(on && l[u] == c1));
            const float c2 = K == 1 ? -1.0f : og_wave_max(lane == k1 ? -INFINITY : l[u]);
            const float mg = c1 - c2;
            int slot = -1, w = 1, acc_id = -1;
            float cf = nan, mo = nan;
            if (!bad) {                                    // (k1 is a valid lane: the row is finite, so its maximum is met)
                const float thr = __shfl(my_thr, k1, 64);
                const int id1 = __shfl(my_id, k1, 64);
                cf = c1;
                mo = mg;
                if (a.c.weight) w = 1 + (int)rintf(fminf(mg, 2.0f) * OG_WEIGHT_SCALE);      // (cosines: mg <= 2 as it is)
                if (c1 >= thr && mg >= a.c.min_margin) {
                    slot = k1;
                    acc_id = id1;
                }
            }
            if (lane == 0) {
                row_slot[j] = slot;
                row_w[j] = w;
                a.accepted[r0 + j] = acc_id;
                if (a.conf) a.conf[r0 + j] = cf;
                if (a.margin) a.margin[r0 + j] = mo;
            }
        }
    }

    // ---- pass 2: ring, candidate and command in window order
    const int V = a.c.vote;
    int head = st->head, len = st->len;
    if (head < 0 || head >= V || len < 0 || len > V) {     // a ring kept under another vote length: start empty
        head = 0;
        len = 0;
    }
    for (int i = lane; i < V; i += 64) {
        ring_slot[i] = st->ring_slot[i];
        ring_w[i] = st->ring_w[i];
    }
    __syncthreads();
    int cnt = 0, sum = 0;                                  // of slot `lane` over the ring
    for (int i = 0; i < len; ++i) {
        const int p = (head + V - len + i) % V;
        if (ring_slot[p] == lane) {
            ++cnt;
            sum += ring_w[p];
        }
    }
    int command = st->command - 1, pending = st->pending, run = st->run;
    for (int j = 0; j < M; ++j) {
        const int sj = row_slot[j], wj = row_w[j];
        if (len == V) {
            if (ring_slot[head] == lane) {
                --cnt;
                sum -= ring_w[head];
            }
        } else {
            ++len;
        }
        if (sj == lane) {
            ++cnt;
            sum += wj;
        }
        __builtin_amdgcn_wave_barrier();                   // (one wave: its LDS reads of ring[head] are ahead of the write)
        if (lane == 0) {
            ring_slot[head] = sj;
            ring_w[head] = wj;
        }
        head = head + 1 == V ? 0 : head + 1;
        const bool qual = on && cnt >= a.c.min_votes;
        const int best = og_wave_max(qual ? sum : -1);
        const unsigned long long who = __ballot(qual && sum == best);
        const int cand = who ? og_first(who) : -1;         // ties: the smallest slot
        const int cand_id = cand >= 0 ? __shfl(my_id, cand, 64) : -1;
        if (cand_id == command || (cand < 0 && a.c.release == 0)) {
            run = 0;
        } else if (run > 0 && cand == pending) {
            ++run;
        } else {
            pending = cand;
            run = 1;
        }
        if (run > 0 && run >= (pending >= 0 ? a.c.dwell : a.c.release)) {
            command = pending >= 0 ? __shfl(my_id, pending, 64) : -1;
            run = 0;
        }
        if (lane == 0) row_cmd[j] = command;
    }
    __syncthreads();
    for (int j = lane; j < M; j += 64) a.command[r0 + j] = row_cmd[j];
    for (int i = lane; i < V; i += 64) {
        st->ring_slot[i] = ring_slot[i];
        st->ring_w[i] = ring_w[i];
    }
    if (lane == 0) {
        st->head = head;
        st->len = len;
        st->command = command + 1;
        st->pending = pending;
        st->run = run;
    }
}

struct OgClassArgs {
    int ids[OG_MAXK];
    float min_cosine[OG_MAXK];
    int K;
};

// installs ids and thresholds; ring and pending empty; the command stays if its class id is among the new ids
__global__ __launch_bounds__(64) void og_set_classes_kernel(OgState* st, OgClassArgs c) {
    const int lane = threadIdx.x;
    const bool on = lane < c.K;
    const int cmd = st->command;
    const bool kept = __ballot(on && cmd > 0 && c.ids[lane] + 1 == cmd) != 0ull;
    st->ids[lane] = on ? c.ids[lane] : -1;
    st->min_cosine[lane] = on ? c.min_cosine[lane] : 0.f;
    if (lane == 0) {
        st->K = c.K;
        st->head = 0;
        st->len = 0;
        st->pending = -1;
        st->run = 0;
        if (!kept) st->command = 0;
    }
}

// ring, pending and command of streams first .. first + gridDim.x - 1 to none; classes and thresholds stay
__global__ __launch_bounds__(64) void og_reset_kernel(OgState* states, int first) {
    OgState* st = states + first + blockIdx.x;
    if (threadIdx.x == 0) {
        st->head = 0;
        st->len = 0;
        st->command = 0;
        st->pending = -1;
        st->run = 0;
    }
}
