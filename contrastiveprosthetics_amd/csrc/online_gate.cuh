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
//   og_rows_kernel, og_sweep_kernel   the gate sweep (cp_online_gate_sweep): many settings over one recording, see below.
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

// The part of a row that no setting enters (include/cpnative.h, "row"): lane k holds the logit of slot k (`on`: k < K).  Returns
// k1, the slot of the first maximum, with c1 = its logit and mg = c1 - runner-up (K = 1: c1 + 1); a row with a non-finite logit
// returns -1 and c1 = mg = NaN.  The same on every lane.  og_push_kernel and og_rows_kernel both classify through this function.
__device__ __forceinline__ int og_row(bool on, int K, int lane, float l, float& c1, float& mg) {
#pragma clang fp contract(off)
    const bool bad = __ballot(on && !isfinite(l)) != 0ull;
    c1 = og_wave_max(l);
    const int k1 = og_first(__ballot(on && l == c1));
    const float c2 = K == 1 ? -1.0f : og_wave_max(lane == k1 ? -INFINITY : l);
    mg = c1 - c2;
    if (bad) {                                             // (else k1 is a valid lane: the row is finite, so its maximum is met)
        c1 = mg = __builtin_nanf("");
        return -1;
    }
    return k1;
}

// What the settings make of a classified row: the ring entry (slot = k1 if accepted else -1, integer weight w).  thr is
// min_cosine[k1].  Per lane: og_push_kernel calls it with one row on all lanes, og_sweep_kernel with one row per lane.
__device__ __forceinline__ void og_judge(int k1, float c1, float mg, float thr, int weight, float min_margin, int& slot, int& w) {
#pragma clang fp contract(off)
    slot = -1;
    w = 1;
    if (k1 >= 0) {
        if (weight) w = 1 + (int)rintf(fminf(mg, 2.0f) * OG_WEIGHT_SCALE);      // (cosines: mg <= 2 as it is)
        if (c1 >= thr && mg >= min_margin) slot = k1;
    }
}

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
            float c1, mg;
            const int k1 = og_row(on, K, lane, l[u], c1, mg);
            int slot, w;
            og_judge(k1, c1, mg, __shfl(my_thr, max(k1, 0), 64), a.c.weight, a.c.min_margin, slot, w);
            const int acc_id = slot >= 0 ? __shfl(my_id, slot, 64) : -1;
            if (lane == 0) {
                row_slot[j] = slot;
                row_w[j] = w;
                a.accepted[r0 + j] = acc_id;
                if (a.conf) a.conf[r0 + j] = c1;
                if (a.margin) a.margin[r0 + j] = mg;
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

// ---------------------------------------------------------------------------------------------------------------------------
// gate sweep (cp_online_gate_sweep): G settings over one recording of n_rows windows, scored against the cues on the device
//
//   og_rows_kernel    what a row is before any setting looks at it (og_row: k1, c1, margin), once per row: 12 bytes in scratch.
//   og_sweep_kernel   one wave per setting, OG_SWEEP_WAVES waves per workgroup, each from the zero gate state.  The wave takes
//                     64 rows at a time, one row per lane: og_judge gives every row's ring entry at once, and the entry that
//                     leaves the ring at row r is the one of row r - vote, which is either in the same 64 rows (a lane
//                     shuffle) or in the wave's ring in LDS at position r % vote (from a zero state head is r % vote).  So both
//                     are known before the walk, and the walk over the 64 rows -- lane k keeps count and weight sum of slot k,
//                     the candidate is a wave maximum, command / pending / run and the ten counters are wave-uniform -- reads
//                     lanes and touches no memory.  A row that neither brings nor removes an accepted entry leaves the
//                     candidate as it was.  Commands leave 64 at a time, the counters once at the end.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int OG_SWEEP_WAVES = 4;        // waves (settings) per workgroup: one per SIMD of a CU, 8 KB of LDS
constexpr int OG_SCORES = 10;            // CP_ONLINE_GATE_SCORES, in the order of score_commands
constexpr int OG_ROWS_PER_WAVE = 4;      // og_rows_kernel: rows a wave classifies, their loads in flight together

struct OgRow {                           // 12 bytes per row
    int k1;                              // slot of the first maximum; -1: a non-finite row
    float c1, margin;
};

__global__ __launch_bounds__(256) void og_rows_kernel(const float* __restrict__ logits, int ldl, long long n_rows, int K,
                                                      OgRow* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const long long r0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * OG_ROWS_PER_WAVE;
    const bool on = lane < K;
    float l[OG_ROWS_PER_WAVE];
#pragma unroll
    for (int u = 0; u < OG_ROWS_PER_WAVE; ++u) l[u] = on && r0 + u < n_rows ? logits[(size_t)(r0 + u) * ldl + lane] : -INFINITY;
#pragma unroll
    for (int u = 0; u < OG_ROWS_PER_WAVE; ++u) {
        if (r0 + u >= n_rows) break;                       // (uniform over the wave)
        OgRow o;
        o.k1 = og_row(on, K, lane, l[u], o.c1, o.margin);
        if (lane == 0) rows[r0 + u] = o;
    }
}

struct OgSweepArgs {
    const OgRow* rows;                   // [n_rows]
    const int32_t* expected;             // [n_rows] slot, -1 rest, -2 (or anything else negative) ignore
    const OgConfig* configs;             // [n_configs], on the device: not checked by the host
    const float* min_cosine;             // [n_configs][64]
    long long n_rows;
    int n_configs, K;
    long long* scores;                   // [n_configs][OG_SCORES]
    int32_t* commands;                   // optional [n_configs][n_rows] slot or -1
};

__global__ __launch_bounds__(64 * OG_SWEEP_WAVES) void og_sweep_kernel(OgSweepArgs a) {
#pragma clang fp contract(off)
    __shared__ int ring_slot_all[OG_SWEEP_WAVES][OG_MAXVOTE], ring_w_all[OG_SWEEP_WAVES][OG_MAXVOTE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * OG_SWEEP_WAVES + wave;
    if (g >= a.n_configs) return;                          // (no workgroup barrier below: the waves do not meet)
    int* ring_slot = ring_slot_all[wave];
    int* ring_w = ring_w_all[wave];
    const OgConfig c = a.configs[g];
    long long* out = a.scores + (size_t)g * OG_SCORES;
    if (c.vote < 1 || c.vote > OG_MAXVOTE || c.min_votes < 1 || c.dwell < 1 || c.release < 0) {
        if (lane < OG_SCORES) out[lane] = -1;              // a setting the gate does not have: nothing is indexed with it
        return;
    }
    const int V = c.vote, K = a.K;
    const bool on = lane < K;
    const float my_thr = on ? a.min_cosine[(size_t)g * OG_MAXK + lane] : 0.f;

    int cnt = 0, sum = 0;                                  // of slot `lane` over the ring
    int cand = -1;                                         // (an empty ring has no candidate: min_votes >= 1)
    int command = -1, pending = -1, run = 0;
    long long n_cue = 0, n_rest = 0, hit = 0, wrong = 0, false_active = 0, switches = 0, segments = 0, reached = 0,
              latency_sum = 0, wrong_segments = 0;
    int seg_e = -1;                                        // expected of the segment the previous row was in; -1: in none
    long long seg_start = 0;
    bool seg_hit = false, seg_wrong = false;

    int head = 0;                                          // base % V: where the ring takes the block's first row
    for (long long base = 0; base < a.n_rows; base += 64, head = (head + 64) % V) {
        const int nb = (int)min((long long)64, a.n_rows - base);
        const long long r = base + lane;
        // ---- the 64 rows at once: entry in, entry out
        int k1 = -1, e = -2;
        float c1 = 0.f, mg = 0.f;
        if (lane < nb) {
            const OgRow row = a.rows[r];
            k1 = row.k1 < K ? row.k1 : -1;
            c1 = row.c1;
            mg = row.margin;
            e = a.expected[r];
        }
        int s_in, w_in;
        og_judge(k1, c1, mg, __shfl(my_thr, max(k1, 0), 64), c.weight, c.min_margin, s_in, w_in);
        // the entry of row r - V leaves: of these 64 rows (lane - V), or of an earlier block (the ring, position r % V)
        const int p = (head + lane) % V;
        int s_out = __shfl(s_in, max(lane - V, 0), 64), w_out = __shfl(w_in, max(lane - V, 0), 64);
        if (lane < V) {
            s_out = -1;                                    // (r < V: nothing leaves yet)
            w_out = 0;
            if (r >= V && lane < nb) {
                s_out = ring_slot[p];
                w_out = ring_w[p];
            }
        }
        __builtin_amdgcn_wave_barrier();                   // (one wave: its LDS reads are ahead of the writes)
        if (lane < nb && lane + V >= nb) {                 // the last row of the block at this ring position
            ring_slot[p] = s_in;
            ring_w[p] = w_in;
        }
        __builtin_amdgcn_wave_barrier();

        // ---- the walk in window order
        int my_cmd = -1;
        for (int j = 0; j < nb; ++j) {
            const int sj = __builtin_amdgcn_readlane(s_in, j), so = __builtin_amdgcn_readlane(s_out, j);
            const int ej = __builtin_amdgcn_readlane(e, j);
            if (sj >= 0 || so >= 0) {                      // (else count and sum of every slot stay, and so does the candidate)
                const int wj = __builtin_amdgcn_readlane(w_in, j), wo = __builtin_amdgcn_readlane(w_out, j);
                if (so == lane) {
                    --cnt;
                    sum -= wo;
                }
                if (sj == lane) {
                    ++cnt;
                    sum += wj;
                }
                const bool qual = on && cnt >= c.min_votes;
                const int best = og_wave_max(qual ? sum : -1);
                const unsigned long long who = __ballot(qual && sum == best);
                cand = who ? og_first(who) : -1;           // ties: the smallest slot
            }
            if (cand == command || (cand < 0 && c.release == 0)) {
                run = 0;
            } else if (run > 0 && cand == pending) {
                ++run;
            } else {
                pending = cand;
                run = 1;
            }
            const int before = command;
            if (run > 0 && run >= (pending >= 0 ? c.dwell : c.release)) {
                command = pending;
                run = 0;
            }
            if (lane == j) my_cmd = command;
            // ---- the score (score_commands in online.py is its definition)
            switches += command != before;
            if (ej >= 0) {
                if (ej != seg_e) {
                    ++segments;
                    seg_e = ej;
                    seg_start = base + j;
                    seg_hit = seg_wrong = false;
                }
                ++n_cue;
                if (command == ej) {
                    ++hit;
                    if (!seg_hit) {
                        seg_hit = true;
                        ++reached;
                        latency_sum += base + j - seg_start;
                    }
                } else if (command >= 0) {
                    ++wrong;
                    if (!seg_wrong) {
                        seg_wrong = true;
                        ++wrong_segments;
                    }
                }
            } else {
                seg_e = -1;
                if (ej == -1) {
                    ++n_rest;
                    false_active += command != -1;
                }
            }
        }
        if (a.commands && lane < nb) a.commands[(size_t)g * a.n_rows + r] = my_cmd;
    }
    const long long s[OG_SCORES] = {n_cue, n_rest, hit, wrong, false_active, switches, segments, reached, latency_sum, wrong_segments};
#pragma unroll
    for (int i = 0; i < OG_SCORES; ++i)
        if (lane == i) out[i] = s[i];
}
