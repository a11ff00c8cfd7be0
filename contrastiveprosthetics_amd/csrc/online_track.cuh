// Prototype tracking (include/cpnative.h, cp_online_track_*): class rows that follow the user between enrolments.  A stage
// behind the decoders, as the gate is: it reads the z / |z| their tails emit on request (the embeddings of a push) and keeps
// per stream, in a workspace of its own (OtState), the enrolled rows (anchor), the current rows, a float64 tracked direction
// per class and a vote ring.  track_reference of contrastiveprosthetics_amd/track.py is the definition; the device equals it
// in every integer and bit.
//
//   ot_push_kernel    grid n_streams, one wave each; lane k serves class slot k and keeps row[k] and anchor[k] in registers.
//                     The push's embeddings (<= 256 x 64 B) and the accumulators (64 x 16 doubles) are staged in LDS.  The
//                     rows are walked in window order through ot_step, because window j's update changes window j + 1's
//                     logits; pred, voted and updated leave LDS in coalesced stores, the state in plain vector stores.
//   ot_step           one window: the tail's logits against the current rows, first maximum and runner-up as wave maxima of
//                     (value, 255 - lane) keys, the decoders' vote ring (ol_vote_step), the acceptance test, and on lane k1
//                     alone the sixteen float64 updates, the norm and the candidate row, in a fixed order.
//   ot_sweep_kernel   cp_online_track_sweep: one wave per setting over one recording, each from a fresh tracker, through
//                     the same ot_step; embeddings and cues come through LDS 64 rows at a time; eight counters per setting.
//   ot_set_rows_kernel, ot_reset_kernel   one wave per stream.
// Everything is integer, single f32 or single f64 operations with floating-point contraction off and no atomics: a stream's
// outputs are the same for any cutting of its rows into calls and for any set of streams that share a launch.
#pragma once
#include "online.cuh"

constexpr int OT_MAXK = 64;              // class slots (CP_ONLINE_MAX_CLASSES): one per lane
constexpr int OT_MAXVOTE = 256;          // ring length (CP_ONLINE_MAX_VOTE)
constexpr int OT_MAXM = 256;             // rows of one stream per push (CP_ONLINE_MAX_WINDOWS)
constexpr int OT_D = 16;                 // embedding width (CP_D_E)
constexpr int OT_SCORES = 8;             // CP_ONLINE_TRACK_SCORES
constexpr int OT_SWEEP_WAVES = 4;        // waves (settings) per workgroup of the sweep: one per SIMD of a CU

// Per-stream state.  A zeroed state is a valid start: no classes, empty ring.
struct OtState {
    int K;                               // ---- class part
    int head, len;                       // ---- ring position and fill
    int pad;
    int ids[OT_MAXK];                    // class id of each slot, ascending, >= 0
    int ring[OT_MAXVOTE];                // slot of each window's first maximum
    long long n_updates[OT_MAXK], n_refused[OT_MAXK];
    float anchor[OT_MAXK][OT_D];         // the enrolled unit rows
    float row[OT_MAXK][OT_D];            // the current rows
    double acc[OT_MAXK][OT_D];           // the tracked direction
};

struct OtConfig {                        // cp_online_track_config, checked on the host
    int vote, agree;
    double rate;
    float min_cosine, min_margin, min_anchor_cosine;
    int reserved0;
};

// what a lane carries through the walk of one stream (or one setting of the sweep)
struct OtWalk {
    float row[OT_D], anc[OT_D];          // of slot `lane`
    long long n_updates, n_refused;      // of slot `lane`
    int head, len, cnt;                  // the ring; cnt: entries of slot `lane` in it
};

struct OtOut {                           // one window, the same on every lane except l
    int k1, voted, updated;              // slots; updated -1: none
    bool refused;
    float l;                             // this lane's logit
};

__device__ __forceinline__ unsigned long long ot_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// (value, 255 - lane) as one integer that orders as the pair does; -0 counts as +0, as `>` sees it.  A lane that is off or
// holds a NaN gets 0, below every number: `>` never picks a NaN, and lane 0's is dealt with by the caller.
__device__ __forceinline__ unsigned long long ot_key(bool live, float l, int lane) {
    unsigned u = __float_as_uint(l == 0.f ? 0.f : l);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return live ? ((unsigned long long)u << 32) | (unsigned)(255 - lane) : 0ull;
}

// One window (include/cpnative.h, "per window"): e its 16 floats in LDS, acc the stream's [64][16] accumulators in LDS, ring
// its vote ring in LDS.  Called by all 64 lanes of one wave.
__device__ __forceinline__ OtOut ot_step(const OtConfig& c, int K, int lane, OtWalk& w, double* acc, int* ring, const float* e) {
#pragma clang fp contract(off)
    const bool on = lane < K;
    float ev[OT_D];
#pragma unroll
    for (int q = 0; q < OT_D / 4; ++q) {
        const float4 v = *(const float4*)(e + 4 * q);
        ev[4 * q] = v.x; ev[4 * q + 1] = v.y; ev[4 * q + 2] = v.z; ev[4 * q + 3] = v.w;
    }
    float l = 0.f;
#pragma unroll
    for (int d = 0; d < OT_D; ++d) l += ev[d] * w.row[d];
    OtOut o;
    o.l = l;
    const bool bad = __ballot(on && !isfinite(l)) != 0ull;
    // the tail's rule: best = 0, then every later slot whose logit is > the best so far.  A NaN is never >, and nothing is > a
    // NaN in slot 0.
    const bool nan0 = __shfl(l != l ? 1 : 0, 0, 64) != 0;
    const unsigned long long key1 = ot_wave_max(ot_key(on && l == l, l, lane));
    const int k1 = nan0 || key1 == 0ull ? 0 : 255 - (int)(key1 & 255u);
    const float c1 = __shfl(l, k1, 64);
    float c2 = -1.0f;
    if (K > 1) {
        const unsigned long long key2 = ot_wave_max(ot_key(on && l == l && lane != k1, l, lane));
        c2 = key2 == 0ull ? -INFINITY : __shfl(l, 255 - (int)(key2 & 255u), 64);
    }
    const float margin = c1 - c2;
    o.k1 = k1;
    o.voted = ol_vote_step(ring, w.head, w.len, w.cnt, c.vote, k1, lane);
    o.updated = -1;
    o.refused = false;
    const bool eligible = c.rate > 0.0 && !bad && c1 >= c.min_cosine && margin >= c.min_margin && (!c.agree || k1 == o.voted);
    if (eligible) {                                            // (uniform over the wave)
        bool ok = false;
        if (lane == k1) {
            const double beta = c.rate, keep = 1.0 - c.rate;
            double a2[OT_D], n2 = 0.0;
#pragma unroll
            for (int d = 0; d < OT_D; ++d) a2[d] = keep * acc[k1 * OT_D + d] + beta * (double)ev[d];
#pragma unroll
            for (int d = 0; d < OT_D; ++d) n2 += a2[d] * a2[d];
            const double nrm = sqrt(n2);
            float cand[OT_D], ca = 0.f;
#pragma unroll
            for (int d = 0; d < OT_D; ++d) cand[d] = (float)(a2[d] / nrm);
#pragma unroll
            for (int d = 0; d < OT_D; ++d) ca += cand[d] * w.anc[d];
            ok = isfinite(n2) && n2 > 0.0 && ca >= c.min_anchor_cosine;
            if (ok) {
#pragma unroll
                for (int d = 0; d < OT_D; ++d) {
                    acc[k1 * OT_D + d] = a2[d];
                    w.row[d] = cand[d];
                }
            }
            w.n_updates += ok;                                 // (two sums, not a branch: a choice between two members
            w.n_refused += !ok;                                //  becomes an indexed access, which lands in scratch)
        }
        ok = __ballot(ok) != 0ull;
        o.updated = ok ? k1 : -1;
        o.refused = !ok;
    }
    return o;
}

struct OtPushArgs {
    OtState* states;
    const float* emb;                    // [total_rows][16]
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int total_rows, ldl;
    int32_t* pred;                       // [total_rows] class ids
    int32_t* voted;                      // [total_rows]
    float* logits;                       // optional [total_rows][ldl]
    int32_t* updated;                    // [total_rows] class id or -1
    OtConfig c;
};

// the stream's state into the walk: rows and counters to registers, accumulators and ring to LDS
__device__ __forceinline__ void ot_load(const OtState* st, int K, int V, int lane, OtWalk& w, double* acc, int* ring) {
    const bool on = lane < K;
#pragma unroll
    for (int q = 0; q < OT_D / 4; ++q) {
        const float4 r = on ? *(const float4*)(st->row[lane] + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = on ? *(const float4*)(st->anchor[lane] + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        w.row[4 * q] = r.x; w.row[4 * q + 1] = r.y; w.row[4 * q + 2] = r.z; w.row[4 * q + 3] = r.w;
        w.anc[4 * q] = a.x; w.anc[4 * q + 1] = a.y; w.anc[4 * q + 2] = a.z; w.anc[4 * q + 3] = a.w;
    }
    w.n_updates = on ? st->n_updates[lane] : 0;
    w.n_refused = on ? st->n_refused[lane] : 0;
    for (int i = lane; i < K * OT_D; i += 64) acc[i] = (&st->acc[0][0])[i];
    w.head = st->head;
    w.len = st->len;
    if (w.head < 0 || w.head >= V || w.len < 0 || w.len > V) {       // a ring kept under another vote length: start empty
        w.head = 0;
        w.len = 0;
    }
    for (int i = lane; i < V; i += 64) ring[i] = st->ring[i];
    __builtin_amdgcn_wave_barrier();
    w.cnt = 0;
    for (int i = 0; i < w.len; ++i) w.cnt += ring[(w.head + V - w.len + i) % V] == lane;
}

__global__ __launch_bounds__(64) void ot_push_kernel(OtPushArgs a) {
    __shared__ __attribute__((aligned(16))) float es[OT_MAXM * OT_D];
    __shared__ double acc[OT_MAXK * OT_D];
    __shared__ int ring[OT_MAXVOTE];
    __shared__ int row_pred[OT_MAXM], row_voted[OT_MAXM], row_upd[OT_MAXM];
    OtState* st = a.states + blockIdx.x;
    const int lane = threadIdx.x;
    const int K = st->K, M = a.m[blockIdx.x], r0 = a.row0[blockIdx.x], V = a.c.vote;
    // a stream without classes, or whose rows disagree with the limits, is left untouched
    if (K < 1 || K > OT_MAXK || M < 1 || M > OT_MAXM || r0 < 0 || r0 > a.total_rows - M) return;
    if (a.logits && K > a.ldl) return;
    const bool on = lane < K;
    const int my_id = on ? st->ids[lane] : -1;
    OtWalk w;
    ot_load(st, K, V, lane, w, acc, ring);
    const float4* src = (const float4*)(a.emb + (size_t)r0 * OT_D);
    for (int i = lane; i < M * (OT_D / 4); i += 64) ((float4*)es)[i] = src[i];
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        const OtOut o = ot_step(a.c, K, lane, w, acc, ring, es + j * OT_D);
        if (a.logits && on) a.logits[(size_t)(r0 + j) * a.ldl + lane] = o.l;
        const int pid = __shfl(my_id, o.k1, 64), vid = __shfl(my_id, o.voted, 64);
        const int uid = o.updated >= 0 ? __shfl(my_id, o.updated, 64) : -1;
        if (lane == 0) {
            row_pred[j] = pid;
            row_voted[j] = vid;
            row_upd[j] = uid;
        }
    }
    __syncthreads();
    for (int j = lane; j < M; j += 64) {
        a.pred[r0 + j] = row_pred[j];
        a.voted[r0 + j] = row_voted[j];
        a.updated[r0 + j] = row_upd[j];
    }
    if (on) {
#pragma unroll
        for (int q = 0; q < OT_D / 4; ++q)
            *(float4*)(st->row[lane] + 4 * q) = make_float4(w.row[4 * q], w.row[4 * q + 1], w.row[4 * q + 2], w.row[4 * q + 3]);
        st->n_updates[lane] = w.n_updates;
        st->n_refused[lane] = w.n_refused;
    }
    for (int i = lane; i < K * OT_D; i += 64) (&st->acc[0][0])[i] = acc[i];
    for (int i = lane; i < V; i += 64) st->ring[i] = ring[i];
    if (lane == 0) {
        st->head = w.head;
        st->len = w.len;
    }
}

struct OtIds {
    int ids[OT_MAXK];
    int K;
};

// installs ids and the anchor (rows, bit for bit); rows and accumulators start at the anchor, counters at 0, the ring empty
__global__ __launch_bounds__(64) void ot_set_rows_kernel(OtState* st, OtIds c, const float* __restrict__ rows) {
    const int lane = threadIdx.x;
    const bool on = lane < c.K;
    st->ids[lane] = on ? c.ids[lane] : -1;
    st->n_updates[lane] = 0;
    st->n_refused[lane] = 0;
    for (int d = 0; d < OT_D; ++d) {
        const float v = on ? rows[lane * OT_D + d] : 0.f;
        st->anchor[lane][d] = v;
        st->row[lane][d] = v;
        st->acc[lane][d] = (double)v;
    }
    if (lane == 0) {
        st->K = c.K;
        st->head = 0;
        st->len = 0;
    }
}

// streams first .. first + gridDim.x - 1: the ring to empty; what != 0: rows and accumulators back to the anchor and the
// counters to 0 as well
__global__ __launch_bounds__(64) void ot_reset_kernel(OtState* states, int first, int what) {
    OtState* st = states + first + blockIdx.x;
    const int lane = threadIdx.x;
    if (what) {
        st->n_updates[lane] = 0;
        st->n_refused[lane] = 0;
        for (int d = 0; d < OT_D; ++d) {
            const float v = st->anchor[lane][d];
            st->row[lane][d] = v;
            st->acc[lane][d] = (double)v;
        }
    }
    if (lane == 0) {
        st->head = 0;
        st->len = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// tracker sweep (cp_online_track_sweep): G settings over one recording of n_rows embeddings, scored against the cues
// ---------------------------------------------------------------------------------------------------------------------------
struct OtSweepArgs {
    const float* emb;                    // [n_rows][16]
    const int32_t* expected;             // [n_rows] slot, -1 rest, anything else negative: ignore
    const OtConfig* configs;             // [n_configs], on the device: not checked by the host
    const float* rows;                   // [K][16] the anchor every setting starts from
    long long n_rows, tail_from;         // cue rows with ordinal >= tail_from count as the last quarter
    int n_configs, K;
    long long* scores;                   // [n_configs][OT_SCORES]
    int32_t* pred;                       // optional [n_configs][n_rows] slots
    int32_t* voted;                      // optional
    int32_t* updated;                    // optional, slot or -1
};

__global__ __launch_bounds__(64 * OT_SWEEP_WAVES) void ot_sweep_kernel(OtSweepArgs a) {
    __shared__ __attribute__((aligned(16))) float es_all[OT_SWEEP_WAVES][64 * OT_D];
    __shared__ double acc_all[OT_SWEEP_WAVES][OT_MAXK * OT_D];
    __shared__ int ring_all[OT_SWEEP_WAVES][OT_MAXVOTE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * OT_SWEEP_WAVES + wave;
    if (g >= a.n_configs) return;                          // (no workgroup barrier below: the waves do not meet)
    float* es = es_all[wave];
    double* acc = acc_all[wave];
    int* ring = ring_all[wave];
    const OtConfig c = a.configs[g];
    long long* out = a.scores + (size_t)g * OT_SCORES;
    if (c.vote < 1 || c.vote > OT_MAXVOTE || !(c.rate >= 0.0 && c.rate < 1.0)) {
        if (lane < OT_SCORES) out[lane] = -1;              // a setting the tracker does not have: nothing is indexed with it
        return;
    }
    const int K = a.K;
    const bool on = lane < K;
    OtWalk w;
#pragma unroll
    for (int d = 0; d < OT_D; ++d) {
        const float v = on ? a.rows[lane * OT_D + d] : 0.f;
        w.row[d] = v;
        w.anc[d] = v;
        if (on) acc[lane * OT_D + d] = (double)v;
    }
    w.n_updates = w.n_refused = 0;
    w.head = w.len = w.cnt = 0;
    long long n_cue = 0, pred_hit = 0, voted_hit = 0, updates = 0, refused = 0, wrong = 0, pred_tail = 0, voted_tail = 0;
    for (long long base = 0; base < a.n_rows; base += 64) {
        const int nb = (int)min((long long)64, a.n_rows - base);
        __builtin_amdgcn_wave_barrier();                   // (one wave: the previous block's reads of es are ahead of the writes)
        int ex = -2;
        if (lane < nb) {
            const float4* src = (const float4*)(a.emb + (size_t)(base + lane) * OT_D);
#pragma unroll
            for (int q = 0; q < OT_D / 4; ++q) ((float4*)es)[lane * (OT_D / 4) + q] = src[q];
            ex = a.expected[base + lane];
        }
        __builtin_amdgcn_wave_barrier();
        int my_pred = 0, my_voted = 0, my_upd = -1;
        for (int j = 0; j < nb; ++j) {
            const OtOut o = ot_step(c, K, lane, w, acc, ring, es + j * OT_D);
            if (lane == j) {
                my_pred = o.k1;
                my_voted = o.voted;
                my_upd = o.updated;
            }
            const int ej = __builtin_amdgcn_readlane(ex, j);
            if (ej >= -1) {                                // a cue or rest; anything else is not scored
                updates += o.updated >= 0;
                refused += o.refused;
                wrong += o.updated >= 0 && o.updated != ej;
                if (ej >= 0) {
                    const bool tail = n_cue >= a.tail_from;
                    ++n_cue;
                    pred_hit += o.k1 == ej;
                    voted_hit += o.voted == ej;
                    pred_tail += tail && o.k1 == ej;
                    voted_tail += tail && o.voted == ej;
                }
            }
        }
        if (lane < nb) {
            const size_t at = (size_t)g * a.n_rows + base + lane;
            if (a.pred) a.pred[at] = my_pred;
            if (a.voted) a.voted[at] = my_voted;
            if (a.updated) a.updated[at] = my_upd;
        }
    }
    const long long s[OT_SCORES] = {n_cue, pred_hit, voted_hit, updates, refused, wrong, pred_tail, voted_tail};
#pragma unroll
    for (int i = 0; i < OT_SCORES; ++i)
        if (lane == i) out[i] = s[i];
}
