// Grasp drive (include/cpnative.h, cp_online_drive_*): the normalised windows of an online decoder and the class a hand follows
// -> a proportional level per window, and the health of every electrode.  A stage behind the decoders and the gate, shaped as
// the gate is: one state machine per stream in a workspace of its own (OdState), one wave per stream, one launch per push.
//
//   od_push_kernel   grid n_streams, one wave each.  The profile of the stream (spans, weights, ids, rest and range) and its ring
//                    are staged in LDS with all loads in flight together.  The stream's rows are then taken 64 at a time:
//                    pass 1, one row per lane, does what does not depend on the state: the slot of the row's class, the mask of
//                    channels inside their range, the q of every channel (to LDS), the mask of channels that count and the level
//                    the row has while every channel that counts is good.  Pass 2 walks the 64 rows in window order, reading
//                    lanes: lanes 0..11 own a channel (status and run counter), a ballot gives `bad`, and only a row with a bad
//                    channel among those that count sums again, over 16 lanes.  Ring, hysteresis and slew are uniform over the
//                    wave.  The three outputs of the 64 rows leave one row per lane.
//   od_set_profile_kernel, od_reset_kernel   one wave per stream.
// Everything is integer or single f32 operations with floating-point contraction off: the outputs are the same for any
// cutting of a stream's rows into calls and for any set of streams that share a launch.
#pragma once
#include "common.cuh"

constexpr int OD_C = 12;                 // channels (CP_EMG_DIM)
constexpr int OD_MAXK = 64;              // class slots (CP_ONLINE_MAX_CLASSES)
constexpr int OD_MAXSMOOTH = 256;        // ring length (CP_ONLINE_DRIVE_MAX_SMOOTH)
constexpr int OD_MAXM = 256;             // rows of one stream per push (CP_ONLINE_MAX_WINDOWS)
constexpr int OD_ONE = 4096;             // full level (CP_ONLINE_DRIVE_ONE)

// Per-stream state.  A zeroed state is a valid start: no profile, all channels good, ring empty, inactive, out = 0.
struct OdState {
    int K;                               // ---- profile part (survives a reset); 0: no profile
    int head, len;                       // ---- stream part: ring position and fill
    int active, out;
    int bad;                             // mask of the bad channels
    int pad[2];
    int run[16];                         // run counter of each channel ([12..15] unused)
    int ids[OD_MAXK];                    // ---- profile: class id of each slot, ascending, >= 0
    float par[48];                       // rest[16], low[16], high[16] per channel ([12..15] of each unused)
    float span[OD_MAXK * OD_C];          // [slot][channel]
    unsigned char weight[OD_MAXK * OD_C];          // [slot][channel], 0..255
    int ring[OD_MAXSMOOTH];              // the last `smooth` raw levels
};

struct OdConfig {                        // cp_online_drive_config, checked on the host
    int smooth, on_level, off_level, rise, fall, bad_after, good_after;
};

struct OdPushArgs {
    OdState* states;
    const float* windows;                // [total_rows][ldw]
    const int32_t* cls;                  // [total_rows] class id or -1
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int ldw, total_rows;
    float* drive;                        // [total_rows]
    int32_t* active;                     // [total_rows] 0/1
    int32_t* bad;                        // [total_rows] mask
    OdConfig c;
};

// sum over the lanes of each group of 16, on every lane of the group
__device__ __forceinline__ int od_sum16(int v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void od_push_kernel(OdPushArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float s_span[OD_MAXK * OD_C];
    __shared__ __attribute__((aligned(16))) unsigned char s_w[OD_MAXK * OD_C];
    __shared__ __attribute__((aligned(16))) int s_ring[OD_MAXSMOOTH];
    __shared__ int s_ids[OD_MAXK];
    __shared__ float s_par[48];                            // rest, low, high
    __shared__ int s_q[64 * OD_C];                         // q of the 64 rows in flight, [row][channel]
    OdState* st = a.states + blockIdx.x;
    const int lane = threadIdx.x;
    const int K = st->K, M = a.m[blockIdx.x], r0 = a.row0[blockIdx.x], V = a.c.smooth;
    // a stream without a profile, or whose rows disagree with the limits, is left untouched
    if (K < 1 || K > OD_MAXK || M < 1 || M > OD_MAXM || r0 < 0 || r0 > a.total_rows - M || V < 1 || V > OD_MAXSMOOTH || a.ldw < OD_C)
        return;

    // ---- profile, ring, state and the first 64 rows into LDS and registers: every load is issued before the first one is
    // waited for
    int head = st->head, len = st->len, active = st->active != 0, out = st->out, sum = 0;
    if (head < 0 || head >= V || len < 0 || len > V) {     // a ring kept under another smooth length: start empty
        head = 0;
        len = 0;
    }
    int g = -1;                                            // of row base + lane: its class and its window
    float x[OD_C];
    auto load_rows = [&](int base) {
        if (base + lane < M) {
            const size_t r = (size_t)(r0 + base + lane);
            g = a.cls[r];
#pragma unroll
            for (int c = 0; c < OD_C; ++c) x[c] = a.windows[r * a.ldw + c];
        }
    };
    {
        const float4* span4 = (const float4*)st->span;
        const int4* w4 = (const int4*)st->weight;
        const int4* ring4 = (const int4*)st->ring;
        const int n_span4 = K * (OD_C / 4), n_w4 = (K * OD_C + 15) / 16;
        float4 sp[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) sp[u] = lane + 64 * u < n_span4 ? span4[lane + 64 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
        const int4 wt = lane < n_w4 ? w4[lane] : make_int4(0, 0, 0, 0);
        const int4 rg = lane * 4 < V ? ring4[lane] : make_int4(0, 0, 0, 0);
        const int id = lane < K ? st->ids[lane] : -1;
        const float par = lane < 48 ? st->par[lane] : 0.f;
        load_rows(0);
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (lane + 64 * u < n_span4) ((float4*)s_span)[lane + 64 * u] = sp[u];
        if (lane < n_w4) ((int4*)s_w)[lane] = wt;
        ((int4*)s_ring)[lane] = rg;
        const int mine[4] = {rg.x, rg.y, rg.z, rg.w};      // the sum of the ring: recomputed, not stored
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int off = lane * 4 + u - head + len;           // position in the ring -> age, 0: the oldest entry
            off = off < 0 ? off + V : off >= V ? off - V : off;
            if (lane * 4 + u < V && off < len) sum += mine[u];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        s_ids[lane] = id;
        if (lane < 48) s_par[lane] = par;
    }
    bool isbad = lane < OD_C && ((st->bad >> lane) & 1);   // lanes 0..11: the channel's status and run counter
    int run = lane < OD_C ? st->run[lane] : 0;
    __syncthreads();

    for (int base = 0; base < M; base += 64) {
        const int nb = min(64, M - base);
        // ---- pass 1: row base + lane on its own
        int slot = -1, mask = 0, raw_all = 0;              // mask: bits 0..11 inside, bits 16..27 the channels that count
        if (lane < nb) {
            if (g >= 0) {                                  // ids ascending: the first slot with ids[slot] >= g
                int lo = 0, hi = K;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_ids[mid] < g) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < K && s_ids[lo] == g) slot = lo;
            }
            int swq = 0, sw = 0;
#pragma unroll
            for (int c = 0; c < OD_C; ++c) {
                if (isfinite(x[c]) && x[c] >= s_par[16 + c] && x[c] <= s_par[32 + c]) mask |= 1 << c;
                int q = 0;
                if (slot >= 0) {
                    const int w = s_w[slot * OD_C + c];
                    const float span = s_span[slot * OD_C + c];
                    if (w > 0 && span > 0.f) {
                        const float d = x[c] - s_par[c];
                        const float e = d / span;
                        const float f = fminf(fmaxf(e, 0.f), 1.f);         // (fmaxf: NaN -> 0)
                        q = (int)rintf(f * (float)OD_ONE);
                        mask |= 1 << (16 + c);
                        swq += w * q;
                        sw += w;
                    }
                }
                s_q[lane * OD_C + c] = q;
            }
            raw_all = sw ? swq / sw : 0;
        }
        load_rows(base + 64);                              // (the next 64 rows are in flight during the walk)
        __syncthreads();

        // ---- pass 2: health, level, ring, hysteresis and slew in window order
        int my_out = 0, my_active = 0, my_bad = 0;
        for (int j = 0; j < nb; ++j) {
            const int mj = __builtin_amdgcn_readlane(mask, j);
            int raw = __builtin_amdgcn_readlane(raw_all, j);
            if (lane < OD_C) {
                const bool inside = (mj >> lane) & 1;
                run = inside == isbad ? run + 1 : 0;       // a good channel outside, or a bad one inside
                if (run >= (isbad ? a.c.good_after : a.c.bad_after)) {
                    isbad = !isbad;
                    run = 0;
                }
            }
            const int bad = (int)__ballot(isbad);
            const int use = mj >> 16;
            if (bad & use) {                               // (uniform) a channel that counts is bad: the sum without it
                const int sj = __builtin_amdgcn_readlane(slot, j);
                int w = 0, wq = 0;
                if (lane < OD_C && (((use & ~bad) >> lane) & 1)) {
                    w = s_w[sj * OD_C + lane];
                    wq = w * s_q[j * OD_C + lane];
                }
                w = __builtin_amdgcn_readfirstlane(od_sum16(w));
                wq = __builtin_amdgcn_readfirstlane(od_sum16(wq));
                raw = w ? wq / w : 0;
            }
            if (len == V) sum -= s_ring[head];
            else ++len;
            sum += raw;
            __builtin_amdgcn_wave_barrier();               // (one wave: its LDS reads of ring[head] are ahead of the write)
            if (lane == 0) s_ring[head] = raw;
            head = head + 1 == V ? 0 : head + 1;
            const int s = (int)((unsigned)sum / (unsigned)len);
            if (!active && s >= a.c.on_level) active = 1;
            else if (active && s < a.c.off_level) active = 0;
            const int target = active ? s : 0;
            out = target > out ? min(out + a.c.rise, target) : max(out - a.c.fall, target);
            if (lane == j) {
                my_out = out;
                my_active = active;
                my_bad = bad;
            }
        }
        if (lane < nb) {
            const size_t r = (size_t)(r0 + base + lane);
            a.drive[r] = (float)my_out / (float)OD_ONE;
            a.active[r] = my_active;
            a.bad[r] = my_bad;
        }
        __syncthreads();                                   // (s_q is written again by the next 64 rows)
    }

    if (lane * 4 < V) ((int4*)st->ring)[lane] = ((const int4*)s_ring)[lane];
    if (lane < OD_C) st->run[lane] = run;
    const int bad = (int)__ballot(isbad);
    if (lane == 0) {
        st->head = head;
        st->len = len;
        st->active = active;
        st->out = out;
        st->bad = bad;
    }
}

// What one launch of od_set_profile_kernel carries (kernel arguments hold 4 KB): ids, rest and range, and the spans and
// weights of OD_PROFILE_SLOTS slots from `first` on.  Two launches install a profile; slots from K on are zeroed.
constexpr int OD_PROFILE_SLOTS = 32;
struct OdProfileArgs {
    int K, first;
    int ids[OD_MAXK];
    float par[48];
    float span[OD_PROFILE_SLOTS * OD_C];
    unsigned char weight[OD_PROFILE_SLOTS * OD_C];
};

// the stream part of a state to its start: all channels good, ring empty, inactive, out = 0
__device__ __forceinline__ void od_restart(OdState* st, int lane) {
    for (int i = lane; i < OD_MAXSMOOTH; i += 64) st->ring[i] = 0;
    if (lane < 16) st->run[lane] = 0;
    if (lane == 0) {
        st->head = 0;
        st->len = 0;
        st->active = 0;
        st->out = 0;
        st->bad = 0;
    }
}

// installs a part of the profile; the launch with first == 0 also installs ids, rest and range, and restarts the stream
__global__ __launch_bounds__(64) void od_set_profile_kernel(OdState* st, OdProfileArgs p) {
    const int lane = threadIdx.x;
    for (int i = lane; i < OD_PROFILE_SLOTS * OD_C; i += 64) {
        const bool on = p.first + i / OD_C < p.K;
        st->span[p.first * OD_C + i] = on ? p.span[i] : 0.f;
        st->weight[p.first * OD_C + i] = on ? p.weight[i] : (unsigned char)0;
    }
    if (p.first != 0) return;
    st->ids[lane] = lane < p.K ? p.ids[lane] : -1;
    if (lane < 48) st->par[lane] = p.par[lane];
    if (lane == 0) st->K = p.K;
    od_restart(st, lane);
}

// the stream part of streams first .. first + gridDim.x - 1 to its start; the profile stays
__global__ __launch_bounds__(64) void od_reset_kernel(OdState* states, int first) { od_restart(states + first + blockIdx.x, threadIdx.x); }
