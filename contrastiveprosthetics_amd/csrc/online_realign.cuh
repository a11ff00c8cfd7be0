// Cue realignment (include/cpnative.h, cp_online_realign*): the windows of a cued recording and the cue -> the onset and offset
// of every cued movement as the sEMG shows them, and per-window labels moved onto them.  realign_reference of
// contrastiveprosthetics_amd/realign.py is the definition; every output here equals it in every integer.
//
//   or_activity_kernel   one thread per window: a[k] = sum over the 12 channels of clamp(rint((x - base) * gain), 0, 255), two f32
//                        operations without contraction.
//   or_default_kernel    one thread per window: expected[k] = cue[k] where cue[k] < 0, else IGNORE.
//   or_segment_kernel    one workgroup of 4 waves per segment.  The row of the table and the bounds it takes from its neighbours
//                        are checked first; then the region's activity, clamped, becomes its exclusive prefix sums in LDS (a
//                        shuffle scan per wave, 256 windows a round, so lanes read and write consecutive words: no bank
//                        conflicts).  Onsets go round the waves and offsets across the lanes: a lane reads P[f] next to its
//                        neighbours' and P[o] is a broadcast.  A candidate is (flag, p, q, o, f) in 64-bit integers, p/q the
//                        explained sum of squares of the two-level fit; two candidates compare by flag, then p1 q2 against
//                        p2 q1 as 128-bit products (__umul64hi and the low product), then smaller o, then smaller f.  That is
//                        a total order, so the butterfly over the lanes and the pass over the four waves end at the same
//                        candidate for any dealing.  Every thread then knows the result and the workgroup writes [s, r1).
// No atomics and no floating point in or_segment_kernel; nothing here depends on the other segments of a launch.
#pragma once
#include "common.cuh"

constexpr int OR_C = 12;                 // channels (CP_EMG_DIM)
constexpr int OR_MAXREGION = 4096;       // windows of one segment's region (CP_ONLINE_REALIGN_MAX_REGION)
constexpr int OR_MAXACT = 4095;          // largest activity of a window (CP_ONLINE_REALIGN_MAX_ACTIVITY)
constexpr int OR_THREADS = 256;
constexpr int OR_WAVES = OR_THREADS / 64;
constexpr int OR_REST = -1, OR_IGNORE = -2;
constexpr int OR_FOUND = 0, OR_NO_PAIR = 1, OR_NO_CONTRAST = 2, OR_TOO_LONG = 3, OR_BAD_ROW = 4;

struct OrActivityArgs {
    const float* windows;                // [n_rows][ldw]
    int ldw;
    long long n_rows;
    float base[OR_C], gain[OR_C];
    int32_t* activity;                   // [n_rows]
};

__global__ __launch_bounds__(OR_THREADS) void or_activity_kernel(OrActivityArgs a) {
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * OR_THREADS + threadIdx.x;
    if (k >= a.n_rows) return;
    const float* x = a.windows + (size_t)k * a.ldw;
    int sum = 0;
#pragma unroll
    for (int c = 0; c < OR_C; ++c) {
        const float d = x[c] - a.base[c];
        const float v = d * a.gain[c];
        const float r = rintf(v);
        sum += !(r > 0.f) ? 0 : r >= 255.f ? 255 : (int)r;       // (NaN: 0)
    }
    a.activity[k] = sum;
}

struct OrConfig {                        // cp_online_realign_config, checked on the host (min_len, min_rest and guard at most 4097
    int max_lag, max_lead, min_len, min_rest, context, min_contrast, guard;      // there: beyond the region they all mean the same)
};

struct OrArgs {
    const int32_t* activity;             // [n_rows]
    const int32_t* cue;                  // [n_rows]
    int n_rows;
    const int32_t* segments;             // [n_segments][2]
    int n_segments;
    OrConfig c;
    int32_t* expected;                   // [n_rows]
    int32_t* out_segments;               // [n_segments][8]
    long long* out_sums;                 // [n_segments][2]
};

__global__ __launch_bounds__(OR_THREADS) void or_default_kernel(const int32_t* cue, long long n_rows, int32_t* expected) {
    const long long k = (long long)blockIdx.x * OR_THREADS + threadIdx.x;
    if (k >= n_rows) return;
    const int c = cue[k];
    expected[k] = c < 0 ? c : OR_IGNORE;
}

// A pair (o, f), both counted from the region's first window.  flag: -1 no pair, 0 inside the length limits, 1 also at the contrast.
struct OrCand {
    unsigned long long p;
    unsigned q;
    int o, f, flag;
};

// the total order of the choice: a before b
__device__ __forceinline__ bool or_before(const OrCand& a, const OrCand& b) {
    if (a.flag != b.flag) return a.flag > b.flag;
    if (a.flag < 0) return false;
    const unsigned long long ah = __umul64hi(a.p, (unsigned long long)b.q), al = a.p * b.q;
    const unsigned long long bh = __umul64hi(b.p, (unsigned long long)a.q), bl = b.p * a.q;
    if (ah != bh) return ah > bh;
    if (al != bl) return al > bl;
    if (a.o != b.o) return a.o < b.o;
    return a.f < b.f;
}

__device__ __forceinline__ void or_write_row(const OrArgs& a, int i, int s, int e, int r0, int r1, int onset, int offset, int status, int cls,
                                             long long SA, long long SR) {
    int32_t* row = a.out_segments + (size_t)i * 8;
    row[0] = s; row[1] = e; row[2] = r0; row[3] = r1; row[4] = onset; row[5] = offset; row[6] = status; row[7] = cls;
    a.out_sums[(size_t)i * 2] = SA;
    a.out_sums[(size_t)i * 2 + 1] = SR;
}

__global__ __launch_bounds__(OR_THREADS) void or_segment_kernel(OrArgs a) {
    __shared__ int s_P[OR_MAXREGION + 1];
    __shared__ int s_wave[OR_WAVES];
    __shared__ OrCand s_best[OR_WAVES];
    const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int M = a.n_rows;
    // ---- the row and what it takes from its neighbours, before anything is indexed with them (all uniform over the workgroup)
    const int s = a.segments[2 * (size_t)i], e = a.segments[2 * (size_t)i + 1];
    const long long prev_e = i > 0 ? a.segments[2 * (size_t)i - 1] : 0;
    const long long next_s = i + 1 < a.n_segments ? a.segments[2 * (size_t)i + 2] : M;
    if (!(0 <= s && s < e && e <= M && prev_e <= s)) {
        if (t == 0) or_write_row(a, i, s, e, -1, -1, -1, -1, OR_BAD_ROW, -1, 0, 0);
        return;
    }
    const int r0 = (int)max(max((long long)s - a.c.context, prev_e), 0LL);                       // prev_e <= s; a bad one may be < 0
    const int r1 = (int)min((long long)e + a.c.max_lag, min(max(next_s, (long long)e), (long long)M));   // a bad next_s: [e, M]
    const int L = r1 - r0;
    const int cls = a.cue[s];
    if (L > OR_MAXREGION) {
        if (t == 0) or_write_row(a, i, s, e, r0, r1, -1, -1, OR_TOO_LONG, cls, 0, 0);
        return;
    }

    // ---- P[j] = a[r0] + .. + a[r0 + j - 1], activity clamped to 0..4095: at most 4095 * 4096 < 2^24
    int carry = 0;
    if (t == 0) s_P[0] = 0;
    for (int base = 0; base < L; base += OR_THREADS) {
        const int j = base + t;
        int x = j < L ? min(max(a.activity[(size_t)r0 + j], 0), OR_MAXACT) : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < OR_WAVES; ++w) {
            const int v = s_wave[w];
            if (w < wave) before += v;
            total += v;
        }
        if (j < L) s_P[j + 1] = carry + before + x;
        carry += total;
        __syncthreads();
    }

    // ---- the candidates: onsets round the waves, offsets across the lanes
    const int T = s_P[L];
    const int so = s - r0, eo = e - r0;
    const int o_hi = min(so + a.c.max_lag, eo - a.c.min_len);
    OrCand best;
    best.p = 0; best.q = 1; best.o = 0; best.f = 0; best.flag = -1;
    for (int o = so + wave; o <= o_hi; o += OR_WAVES) {
        const int f_lo = max(o + a.c.min_len, eo - a.c.max_lead);
        const int f_hi = min(L, o + L - a.c.min_rest);                                          // n_R = L - (f - o) >= min_rest
        const int Po = s_P[o];
        for (int f = f_lo + lane; f <= f_hi; f += 64) {
            const int nA = f - o, nR = L - nA;
            const long long SA = s_P[f] - Po, SR = T - SA;
            OrCand c;
            c.q = (unsigned)nA * (unsigned)nR;
            c.p = (unsigned long long)(SA * SA) * (unsigned)nR + (unsigned long long)(SR * SR) * (unsigned)nA;    // < 2^61
            c.o = o;
            c.f = f;
            c.flag = SA * nR - SR * nA >= max((long long)a.c.min_contrast * c.q, 1LL);
            if (or_before(c, best)) best = c;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        OrCand other;
        other.p = __shfl_xor(best.p, d, 64);
        other.q = __shfl_xor(best.q, d, 64);
        other.o = __shfl_xor(best.o, d, 64);
        other.f = __shfl_xor(best.f, d, 64);
        other.flag = __shfl_xor(best.flag, d, 64);
        if (or_before(other, best)) best = other;
    }
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    best = s_best[0];
#pragma unroll
    for (int w = 1; w < OR_WAVES; ++w) {
        const OrCand other = s_best[w];
        if (or_before(other, best)) best = other;
    }

    // ---- the row of the tables, and the labels of [s, r1)
    const int status = best.flag < 0 ? OR_NO_PAIR : best.flag == 0 ? OR_NO_CONTRAST : OR_FOUND;
    const long long onset = (long long)r0 + best.o, offset = (long long)r0 + best.f, guard = a.c.guard;
    if (t == 0) {
        const long long SA = best.flag < 0 ? 0 : s_P[best.f] - s_P[best.o];
        or_write_row(a, i, s, e, r0, r1, best.flag < 0 ? -1 : (int)onset, best.flag < 0 ? -1 : (int)offset, status, cls, SA,
                     best.flag < 0 ? 0 : T - SA);
    }
    if (status != OR_FOUND) return;
    for (long long k = (long long)s + t; k < r1; k += OR_THREADS) {
        int v;
        if (k >= onset + guard && k < offset - guard) v = cls;
        else if (k < e) v = (k < onset - guard || k >= offset + guard) ? OR_REST : OR_IGNORE;
        else v = k < offset + guard ? OR_IGNORE : a.cue[k];
        a.expected[k] = v;
    }
}
