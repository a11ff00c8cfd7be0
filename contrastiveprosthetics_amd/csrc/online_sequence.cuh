// Grasp sequence decoder (include/cpnative.h, cp_online_seq_*): fixed-lag Viterbi behind the logits of an online decoder.
// A stage like the gate (csrc/online_gate.cuh): it reads the cosines a push emits and keeps one state per stream in a workspace
// of its own (SqState), so the decoders' kernels and outputs stay as they are and one kernel serves all four of them.
//
//   seq_push_kernel   grid n_streams, one wave each; lane j serves class slot j and holds column j of the cost matrix in
//                     registers; the "none" state is wave-uniform.  Per window: the emission (q(l) - thr, 0 for a row with a
//                     non-finite logit), sq_step, the back-pointer row to the ring in LDS, and the traceback: `lag` dependent
//                     LDS byte reads at a wave-uniform address, the serial part.  The rows' logits are loaded three windows ahead
//                     (they do not depend on the state).  command / now / lead leave LDS in coalesced stores.
//   seq_set_model_kernel, seq_reset_kernel   one wave per stream.
//   seq_rows_kernel, seq_sweep_kernel   the sweep (cp_online_seq_sweep): many (cost matrix, lag, thresholds) over one recording.
// Everything behind q() is int32 arithmetic: the outputs are the same for any cutting of a stream's rows into calls and for any
// set of streams that share a launch.  sq_step is the one step function of the push and of the sweep.
#pragma once
#include "common.cuh"
#include "online_gate.cuh"               // og_wave_max, og_first

constexpr int SQ_MAXK = 64;              // class slots (CP_ONLINE_MAX_CLASSES): one per lane
constexpr int SQ_NONE = 64;              // the "none" state's slot on the device, whatever K is
constexpr int SQ_RING = 64;              // back-pointer rows kept (CP_ONLINE_SEQ_RING): lag <= 63
constexpr int SQ_BP_STRIDE = 68;         // bytes of a back-pointer row: columns 0..63, column 64 (none), 3 unused
constexpr int SQ_MAXM = 256;             // rows of one stream per push (CP_ONLINE_MAX_WINDOWS)
constexpr int SQ_FLOOR = -(1 << 29);     // scores lie in [SQ_FLOOR, 0]
constexpr int SQ_COST_MAX = 1 << 28;     // "as good as forbidden"; costs are clamped into 0..SQ_COST_MAX where they are installed
constexpr int SQ_COL_OFF = 1 << 30;      // col[i] of a slot i >= K: SQ_FLOOR - 2^30 is inside int32 and below every real candidate
constexpr int SQ_N_CAP = 1 << 30;        // n saturates here (it is only ever compared with lag)
constexpr int SQ_BAD_ROW = INT32_MIN;    // seq_rows_kernel: q of a row with a non-finite logit
constexpr float SQ_SCALE = 1048576.f;    // 2^20, the gate's margin scale

// Per-stream state.  A zeroed state is a valid start: no classes.  SequenceGate.state reads it back: keep the layout in step.
struct SqState {
    int K, lag;                          // ---- model part (survives a reset)
    int n, head;                         // ---- stream part: windows seen (saturating), ring row of the next window
    int score_none, c_nn;                // score of none; C[none][none]
    int pad[2];
    int ids[SQ_MAXK];                    // class id of each slot, ascending, >= 0
    int thr[SQ_MAXK];                    // q(min_cosine)
    int c_cn[SQ_MAXK];                   // C[k][none]
    int c_nc[SQ_MAXK];                   // C[none][k]
    int cc[SQ_MAXK][SQ_MAXK];            // C[i][j], class to class
    int score[SQ_MAXK];
    unsigned char bp[SQ_RING][SQ_BP_STRIDE];     // back-pointers: a slot, or SQ_NONE
};

// the gate's margin quantisation: half-even, and the product with 2^20 is exact
__device__ __forceinline__ int sq_q(float x) {
#pragma clang fp contract(off)
    return (int)rintf(fminf(fmaxf(x, -2.0f), 2.0f) * SQ_SCALE);
}

__device__ __forceinline__ int sq_cost(int c) { return min(max(c, 0), SQ_COST_MAX); }

// One window (include/cpnative.h, "step" to "now"): lane j < K (`on`) holds score[j], its emission e and column j of C in
// col[0..K-1] (SQ_COL_OFF behind them; a lane that is not `on` holds score SQ_FLOOR) with c_nc = C[none][j] and c_cn = C[j][none]; score_none and c_nn are wave-uniform.  Updates the scores and returns
// the lane's back-pointer bp, the none column's bp_none, now (slot or SQ_NONE) and lead, the last three the same on every lane.
// The smallest intermediate is -2^29 - 2^28 - 2^22.
__device__ __forceinline__ void sq_step(const int (&col)[SQ_MAXK], int c_cn, int c_nc, int c_nn, int K, int lane, bool on, int e,
                                        int& score, int& score_none, int& bp, int& bp_none, int& now, int& lead) {
    // a class column: predecessors in ascending slot order with a strict >, none last, so the first maximum needs no tie key
    int best = INT32_MIN;
    bp = 0;
#pragma unroll
    for (int i0 = 0; i0 < SQ_MAXK; i0 += 8) {
        if (i0 < K) {                                      // (uniform over the wave; a slot >= K of the block loses: SQ_COL_OFF)
#pragma unroll
            for (int i = i0; i < i0 + 8; ++i) {
                const int v = __builtin_amdgcn_readlane(score, i) - col[i];
                if (v > best) {
                    best = v;
                    bp = i;
                }
            }
        }
    }
    if (score_none - c_nc > best) {
        best = score_none - c_nc;
        bp = SQ_NONE;
    }
    // the none column: a wave maximum, the smallest slot among equals
    const int vn = on ? score - c_cn : INT32_MIN;
    int top = og_wave_max(vn);
    bp_none = og_first(__ballot(on && vn == top));         // (K >= 1: the ballot is not empty)
    if (score_none - c_nn > top) {
        top = score_none - c_nn;
        bp_none = SQ_NONE;
    }
    const int nw = on ? best + e : INT32_MIN;              // new[j]; new[none] = top
    const int mx = max(og_wave_max(nw), top);
    const unsigned long long first = __ballot(on && nw == mx);
    now = first ? og_first(first) : SQ_NONE;
    int second = og_wave_max(lane == now ? INT32_MIN : nw);
    if (now != SQ_NONE) second = max(second, top);         // (K + 1 >= 2 states: `second` is one of them)
    score = on ? max(nw - mx, SQ_FLOOR) : SQ_FLOOR;
    score_none = max(top - mx, SQ_FLOOR);
    lead = -max(second - mx, SQ_FLOOR);
}

// the state `lag` windows back on the best path that ends in `now`: follows `lag` rows of the ring, the newest (row `newest`) first
__device__ __forceinline__ int sq_trace(const unsigned char* bp, int newest, int lag, int now) {
    int s = now;
    for (int t = 0; t < lag; ++t) s = min((int)bp[((newest - t) & (SQ_RING - 1)) * SQ_BP_STRIDE + s], SQ_NONE);    // (min: stays in the row)
    return __builtin_amdgcn_readfirstlane(s);              // (the same on every lane: the callers branch on it)
}

struct SqPushArgs {
    SqState* states;
    const float* logits;                 // [total_rows][ldl]
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int ldl, total_rows;
    int32_t* command;                    // [total_rows] class id or -1
    int32_t* now;                        // optional [total_rows] class id or -1
    int32_t* lead;                       // optional [total_rows]
};

__global__ __launch_bounds__(64) void seq_push_kernel(SqPushArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char bp_ring[SQ_RING * SQ_BP_STRIDE];
    __shared__ int row_cmd[SQ_MAXM], row_now[SQ_MAXM], row_lead[SQ_MAXM];
    SqState* st = a.states + blockIdx.x;
    const int lane = threadIdx.x;
    const int K = st->K, lag = st->lag, M = a.m[blockIdx.x], r0 = a.row0[blockIdx.x];
    // a stream without a model, or whose rows disagree with the limits, is left untouched
    if (K < 1 || K > SQ_MAXK || K > a.ldl || lag < 0 || lag >= SQ_RING || M < 1 || M > SQ_MAXM || r0 < 0 || r0 > a.total_rows - M) return;
    const bool on = lane < K;
    const int my_id = on ? st->ids[lane] : -1;
    const int my_thr = on ? st->thr[lane] : 0;
    int col[SQ_MAXK];
#pragma unroll
    for (int i = 0; i < SQ_MAXK; ++i) col[i] = on && i < K ? st->cc[i][lane] : SQ_COL_OFF;
    const int c_cn = on ? st->c_cn[lane] : 0, c_nc = on ? st->c_nc[lane] : 0, c_nn = st->c_nn;
    int score = on ? max(min(st->score[lane], 0), SQ_FLOOR) : SQ_FLOOR;
    int score_none = max(min(st->score_none, 0), SQ_FLOOR);
    int n = min(max(st->n, 0), SQ_N_CAP), head = st->head & (SQ_RING - 1);
    {
        const int* src = (const int*)&st->bp[0][0];
        int* dst = (int*)bp_ring;
        for (int i = lane; i < SQ_RING * SQ_BP_STRIDE / 4; i += 64) dst[i] = src[i];
    }
    __syncthreads();

    // the rows do not depend on the state: the loads of the next three are in flight behind the one at work
    const float* lrow = a.logits + (size_t)r0 * a.ldl + lane;
    float l0 = on ? lrow[0] : 0.f, l1 = on && 1 < M ? lrow[(size_t)a.ldl] : 0.f, l2 = on && 2 < M ? lrow[(size_t)2 * a.ldl] : 0.f;
    for (int j = 0; j < M; ++j) {
        const float l3 = on && j + 3 < M ? lrow[(size_t)(j + 3) * a.ldl] : 0.f;
        const bool bad = __ballot(on && !isfinite(l0)) != 0ull;
        const int e = on && !bad ? sq_q(l0) - my_thr : 0;
        int bp, bp_none, now, lead;
        sq_step(col, c_cn, c_nc, c_nn, K, lane, on, e, score, score_none, bp, bp_none, now, lead);
        bp_ring[head * SQ_BP_STRIDE + lane] = (unsigned char)(on ? bp : 0);
        if (lane == 0) bp_ring[head * SQ_BP_STRIDE + SQ_NONE] = (unsigned char)bp_none;
        __builtin_amdgcn_wave_barrier();                   // (one wave: the traceback's LDS reads are behind the writes)
        n = min(n + 1, SQ_N_CAP);
        const int s = n > lag ? sq_trace(bp_ring, head, lag, now) : SQ_NONE;
        __builtin_amdgcn_wave_barrier();
        head = (head + 1) & (SQ_RING - 1);
        const int cmd_id = __shfl(my_id, s & 63, 64), now_id = __shfl(my_id, now & 63, 64);
        if (lane == 0) {
            row_cmd[j] = s == SQ_NONE ? -1 : cmd_id;
            row_now[j] = now == SQ_NONE ? -1 : now_id;
            row_lead[j] = lead;
        }
        l0 = l1;
        l1 = l2;
        l2 = l3;
    }
    __syncthreads();
    for (int j = lane; j < M; j += 64) {
        a.command[r0 + j] = row_cmd[j];
        if (a.now) a.now[r0 + j] = row_now[j];
        if (a.lead) a.lead[r0 + j] = row_lead[j];
    }
    {
        int* dst = (int*)&st->bp[0][0];
        const int* src = (const int*)bp_ring;
        for (int i = lane; i < SQ_RING * SQ_BP_STRIDE / 4; i += 64) dst[i] = src[i];
    }
    st->score[lane] = on ? score : 0;
    if (lane == 0) {
        st->score_none = score_none;
        st->n = n;
        st->head = head;
    }
}

struct SqModelArgs {
    int ids[SQ_MAXK];
    int thr[SQ_MAXK];
    int K, lag;
};

// scores, ring and n of one stream to the start
__device__ __forceinline__ void sq_restart(SqState* st, int lane) {
    st->score[lane] = 0;
    int* bp = (int*)&st->bp[0][0];
    for (int i = lane; i < SQ_RING * SQ_BP_STRIDE / 4; i += 64) bp[i] = 0;
    if (lane == 0) {
        st->score_none = 0;
        st->n = 0;
        st->head = 0;
    }
}

// installs ids, thresholds, lag and the cost matrix (cost: (K+1, K+1) int32 on the device, clamped into 0..2^28) and restarts the stream
__global__ __launch_bounds__(64) void seq_set_model_kernel(SqState* st, SqModelArgs c, const int32_t* __restrict__ cost) {
    const int lane = threadIdx.x;
    const int K = c.K, ld = c.K + 1;
    const bool on = lane < K;
    st->ids[lane] = on ? c.ids[lane] : -1;
    st->thr[lane] = on ? c.thr[lane] : 0;
    st->c_cn[lane] = on ? sq_cost(cost[lane * ld + K]) : 0;
    st->c_nc[lane] = on ? sq_cost(cost[K * ld + lane]) : 0;
    for (int i = 0; i < SQ_MAXK; ++i) st->cc[i][lane] = on && i < K ? sq_cost(cost[i * ld + lane]) : 0;
    if (lane == 0) {
        st->K = K;
        st->lag = c.lag;
        st->c_nn = sq_cost(cost[K * ld + K]);
    }
    sq_restart(st, lane);
}

// streams first .. first + gridDim.x - 1 to the start; the model stays
__global__ __launch_bounds__(64) void seq_reset_kernel(SqState* states, int first) { sq_restart(states + first + blockIdx.x, threadIdx.x); }

// ---------------------------------------------------------------------------------------------------------------------------
// sequence sweep (cp_online_seq_sweep): G configs over one recording of n_rows windows, scored against the cues on the device
//
//   seq_rows_kernel    q(l) of every logit, once per row (the part no config enters): 64 int32 per row in scratch, of which the
//                      first K are written; a row with a non-finite logit holds SQ_BAD_ROW in all of them.
//   seq_sweep_kernel   one wave per config, SQ_SWEEP_WAVES waves per workgroup, each from the zero state.  The wave holds its
//                      model's column in registers and its 64 back-pointer rows in LDS, walks the rows in window order through
//                      sq_step and sq_trace, and keeps the ten counters of score_commands wave-uniform.  Commands leave 64 at a
//                      time, the counters once at the end.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SQ_SWEEP_WAVES = 4;        // waves (configs) per workgroup: one per SIMD of a CU, 17 KB of LDS
constexpr int SQ_ROWS_PER_WAVE = 4;      // seq_rows_kernel: rows a wave quantises, their loads in flight together

__global__ __launch_bounds__(256) void seq_rows_kernel(const float* __restrict__ logits, int ldl, long long n_rows, int K,
                                                       int32_t* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const long long r0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * SQ_ROWS_PER_WAVE;
    const bool on = lane < K;
    float l[SQ_ROWS_PER_WAVE];
#pragma unroll
    for (int u = 0; u < SQ_ROWS_PER_WAVE; ++u) l[u] = on && r0 + u < n_rows ? logits[(size_t)(r0 + u) * ldl + lane] : 0.f;
#pragma unroll
    for (int u = 0; u < SQ_ROWS_PER_WAVE; ++u) {
        if (r0 + u >= n_rows) break;                       // (uniform over the wave)
        const bool bad = __ballot(on && !isfinite(l[u])) != 0ull;
        if (on) q[(size_t)(r0 + u) * SQ_MAXK + lane] = bad ? SQ_BAD_ROW : sq_q(l[u]);
    }
}

struct SqSweepConfig {                   // cp_online_seq_config
    int model, lag;
};

struct SqSweepArgs {
    const int32_t* q;                    // [n_rows][64]
    const int32_t* expected;             // [n_rows] slot, -1 rest, -2 (or anything else negative) ignore
    const int32_t* costs;                // [n_models][K + 1][K + 1]
    const SqSweepConfig* configs;        // [n_configs], on the device: not checked by the host
    const float* min_cosine;             // [n_configs][64]
    long long n_rows;
    int n_models, n_configs, K;
    long long* scores;                   // [n_configs][OG_SCORES]
    int32_t* commands;                   // optional [n_configs][n_rows] slot or -1
};

__global__ __launch_bounds__(64 * SQ_SWEEP_WAVES) void seq_sweep_kernel(SqSweepArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char bp_all[SQ_SWEEP_WAVES][SQ_RING * SQ_BP_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * SQ_SWEEP_WAVES + wave;
    if (g >= a.n_configs) return;                          // (no workgroup barrier below: the waves do not meet)
    unsigned char* bp_ring = bp_all[wave];
    const SqSweepConfig c = a.configs[g];
    long long* out = a.scores + (size_t)g * OG_SCORES;
    if (c.lag < 0 || c.lag >= SQ_RING || c.model < 0 || c.model >= a.n_models) {
        if (lane < OG_SCORES) out[lane] = -1;              // a config the stage does not have: nothing is indexed with it
        return;
    }
    const int K = a.K, ld = a.K + 1, lag = c.lag;
    const bool on = lane < K;
    const int32_t* cost = a.costs + (size_t)c.model * ld * ld;
    int col[SQ_MAXK];
#pragma unroll
    for (int i = 0; i < SQ_MAXK; ++i) col[i] = on && i < K ? sq_cost(cost[i * ld + lane]) : SQ_COL_OFF;
    const int c_cn = on ? sq_cost(cost[lane * ld + K]) : 0, c_nc = on ? sq_cost(cost[K * ld + lane]) : 0, c_nn = sq_cost(cost[K * ld + K]);
    const int my_thr = on ? sq_q(a.min_cosine[(size_t)g * SQ_MAXK + lane]) : 0;

    int score = on ? 0 : SQ_FLOOR, score_none = 0;
    int command = -1;
    long long n_cue = 0, n_rest = 0, hit = 0, wrong = 0, false_active = 0, switches = 0, segments = 0, reached = 0,
              latency_sum = 0, wrong_segments = 0;
    int seg_e = -1;                                        // expected of the segment the previous row was in; -1: in none
    long long seg_start = 0;
    bool seg_hit = false, seg_wrong = false;

    for (long long base = 0; base < a.n_rows; base += 64) {
        const int nb = (int)min((long long)64, a.n_rows - base);
        const int ex = lane < nb ? a.expected[base + lane] : -2;
        int my_cmd = -1;
        // the rows do not depend on the state: the loads of the next three are in flight behind the one at work
        const int32_t* qrow = a.q + (size_t)base * SQ_MAXK + lane;
        int q0 = on ? qrow[0] : 0, q1 = on && 1 < nb ? qrow[SQ_MAXK] : 0, q2 = on && 2 < nb ? qrow[2 * SQ_MAXK] : 0;
        for (int j = 0; j < nb; ++j) {                     // j is also the ring row: base is a multiple of 64
            const int q3 = on && j + 3 < nb ? qrow[(j + 3) * SQ_MAXK] : 0;
            const int e = on && q0 != SQ_BAD_ROW ? q0 - my_thr : 0;
            int bp, bp_none, now, lead;
            sq_step(col, c_cn, c_nc, c_nn, K, lane, on, e, score, score_none, bp, bp_none, now, lead);
            bp_ring[j * SQ_BP_STRIDE + lane] = (unsigned char)(on ? bp : 0);
            if (lane == 0) bp_ring[j * SQ_BP_STRIDE + SQ_NONE] = (unsigned char)bp_none;
            __builtin_amdgcn_wave_barrier();           // (one wave: the traceback's LDS reads are behind the writes)
            const int s = base + j >= lag ? sq_trace(bp_ring, j, lag, now) : SQ_NONE;
            __builtin_amdgcn_wave_barrier();
            const int before = command;
            command = s == SQ_NONE ? -1 : s;
            if (lane == j) my_cmd = command;
            // ---- the score (score_commands in online.py is its definition), as og_sweep_kernel keeps it
            const int ej = __builtin_amdgcn_readlane(ex, j);
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
            q0 = q1;
            q1 = q2;
            q2 = q3;
        }
        if (a.commands && lane < nb) a.commands[(size_t)g * a.n_rows + base + lane] = my_cmd;
    }
    const long long s[OG_SCORES] = {n_cue, n_rest, hit, wrong, false_active, switches, segments, reached, latency_sum, wrong_segments};
#pragma unroll
    for (int i = 0; i < OG_SCORES; ++i)
        if (lane == i) out[i] = s[i];
}
