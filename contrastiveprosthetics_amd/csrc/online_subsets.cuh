// Grasp-set search (include/cpnative.h, cp_online_subset_sweep): many class subsets of one cued recording, each scored as the
// decoders would decode it if the user kept that subset only.  `score_subset` of contrastiveprosthetics_amd/online.py is the
// definition; the two kernels restate it in integers (the only floating-point operations are comparisons of logits).
//
//   os_rows_kernel    what a row is before any subset looks at it, once per row: its slots in descending logit order (ties
//                     ascending by slot) as 64 bytes, the places behind K filled with 0xFF.  One wave per row, lane k = slot k; a
//                     lane's place is the number of lanes that beat it.  A row with a non-finite logit is 64 times 0xFF: no
//                     subset finds a slot in it, which is its prediction "none".
//   os_sweep_kernel   one wave per subset, OS_WAVES waves per workgroup, no workgroup barrier.  The wave takes 64 rows at a
//                     time, one row per lane: a row is kept if its cue is negative or a slot of the subset, and the raw
//                     prediction of a kept row is the first byte of its order whose bit is set in the (wave-uniform) mask.  The
//                     kept rows are packed to the low lanes through LDS, so that lane i holds the i-th kept row of the block
//                     and the ring runs in kept-row order: the entry that leaves with kept row q is that of kept row q - vote,
//                     which is in the same block (a lane shuffle) or in the wave's ring in LDS at q % vote.  Both are known
//                     before the walk.  The walk visits only rows that change the ring's counts or carry a cue: lane k keeps the
//                     count of slot k over the ring and the voted hits and cue rows of class k; the vote is the largest count,
//                     smallest slot first, found bit by bit with ballots (a count is at most `vote`).  Scalar counters and
//                     worst_* leave once per subset.
#pragma once
#include "online_gate.cuh"

constexpr int OS_WAVES = 4;              // waves (subsets) per workgroup: one per SIMD of a CU, 5 KB of LDS
constexpr int OS_SCORES = 7;             // CP_ONLINE_SUBSET_SCORES, in the order of SUBSET_SCORE_KEYS
constexpr int OS_ORDER = 64;             // bytes of a row's order in scratch
constexpr int OS_NONE = 0xFF;            // an order byte that names no slot

__global__ __launch_bounds__(256) void os_rows_kernel(const float* __restrict__ logits, int ldl, long long n_rows, int K,
                                                      unsigned char* __restrict__ order) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;                               // (uniform over the wave)
    const bool on = lane < K;
    const float l = on ? logits[(size_t)r * ldl + lane] : 0.f;
    const bool bad = __ballot(on && !isfinite(l)) != 0ull;
    int place = 0;                                         // lanes that beat this one: a larger logit, or the same and a lower slot
    for (int j = 0; j < K; ++j) {
        const float lj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l), j));
        place += (lj > l || (lj == l && j < lane)) ? 1 : 0;
    }
    unsigned char* o = order + (size_t)r * OS_ORDER;
    if (bad || !on)
        o[lane] = OS_NONE;                                 // (a finite row: the places of its K slots are 0..K-1, each once)
    else
        o[place] = (unsigned char)lane;
}

struct OsSweepArgs {
    const unsigned char* order;          // [n_rows][OS_ORDER]
    const int32_t* expected;             // [n_rows] slot; negative, or >= K: kept and not scored
    const unsigned long long* subsets;   // [n_subsets] bit k = slot k, on the device: not checked by the host
    long long n_rows;
    int n_subsets, K, vote;
    long long* scores;                   // [n_subsets][OS_SCORES]
    int32_t* class_hits;                 // optional [n_subsets][64]
};

// the slot with the largest count, the smallest such slot, or -1 if every count is 0; counts are below 2^(top+1).  The same on
// every lane.
__device__ __forceinline__ int os_vote(int cnt, int top) {
    unsigned long long alive = ~0ull;
    bool any = false;
    for (int b = top; b >= 0; --b) {
        const unsigned long long m = __ballot((cnt >> b) & 1) & alive;
        if (m) {
            alive = m;
            any = true;
        }
    }
    return any ? og_first(alive) : -1;
}

__global__ __launch_bounds__(64 * OS_WAVES) void os_sweep_kernel(OsSweepArgs a) {
    __shared__ int ring_all[OS_WAVES][OG_MAXVOTE];
    __shared__ int pack_all[OS_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * OS_WAVES + wave;
    if (g >= a.n_subsets) return;                          // (no workgroup barrier below: the waves do not meet)
    int* ring = ring_all[wave];
    int* pack = pack_all[wave];
    const int K = a.K, V = a.vote;
    const unsigned long long mask = a.subsets[g];
    long long* out = a.scores + (size_t)g * OS_SCORES;
    if (mask == 0ull || (K < 64 && (mask >> K) != 0ull)) {
        if (lane < OS_SCORES) out[lane] = -1;              // no subset of these classes: nothing is indexed with it
        return;
    }
    const int top = 31 - __clz(V);                         // a count is at most V
    const int n_chunks = (K + 15) >> 4;                    // 16-byte pieces of an order that hold slots

    int cnt = 0;                                           // of slot `lane` over the ring
    int voted = -1;
    int class_n = 0, class_hit = 0;                        // cue rows of class `lane`, and those whose vote is that class
    long long n_cue = 0, hit = 0, voted_hit = 0;
    int head = 0;                                          // kept rows so far, modulo V: where the ring takes the next one
    bool full = false;                                     // V or more rows kept before this block

    for (long long base = 0; base < a.n_rows; base += 64) {
        const int nb = (int)min((long long)64, a.n_rows - base);
        const long long r = base + lane;
        // ---- the 64 rows at once: kept or dropped, and the raw prediction of the kept ones
        int e = -1, pred = -1;
        bool kept = false;
        if (lane < nb) {
            e = a.expected[r];
            if (e < 0 || e >= K) e = -1;                   // not scored
            kept = e < 0 || ((mask >> e) & 1ull) != 0ull;
        }
        if (kept) {
            const uint4* o = (const uint4*)(a.order + (size_t)r * OS_ORDER);
            for (int c = 0; c < n_chunks && pred < 0; ++c) {
                const uint4 q = o[c];
                const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int b = 15; b >= 0; --b) {            // (downwards: the first byte that is in the subset is assigned last)
                    const unsigned s = (w[b >> 2] >> (8 * (b & 3))) & 0xFFu;
                    if (s < 64u && ((mask >> s) & 1ull) != 0ull) pred = (int)s;
                }
            }
        }
        const unsigned long long km = __ballot(kept);
        const int nk = __popcll(km);
        if (nk == 0) continue;                             // (uniform over the wave)
        // ---- pack the kept rows to lanes 0 .. nk-1, in row order
        const int rank = __popcll(km & ((1ull << lane) - 1ull));
        __builtin_amdgcn_wave_barrier();                   // (one wave: the reads of the block before are ahead of these writes)
        if (kept) pack[rank] = (pred + 1) | ((e + 1) << 8);
        __builtin_amdgcn_wave_barrier();
        const int pk = lane < nk ? pack[lane] : 0;
        const int s_in = (pk & 0xFF) - 1, ec = (pk >> 8) - 1;          // lanes nk..63: none, not scored
        // the entry of kept row q - V leaves with kept row q: of this block (lane - V), or of an earlier one (the ring, q % V)
        const int p = (head + lane) % V;
        int s_out = __shfl(s_in, max(lane - V, 0), 64);
        if (lane < V) {
            s_out = -1;                                    // (fewer than V rows kept so far: nothing leaves yet)
            if (lane < nk && (full || head + lane >= V)) s_out = ring[p];
        }
        __builtin_amdgcn_wave_barrier();                   // (one wave: its LDS reads are ahead of the writes)
        if (lane < nk && lane + V >= nk) ring[p] = s_in;   // the last kept row of the block at this ring position
        __builtin_amdgcn_wave_barrier();

        // ---- what needs no order
        const bool cue = lane < nk && ec >= 0;
        n_cue += __popcll(__ballot(cue));
        hit += __popcll(__ballot(cue && s_in == ec));
        // ---- the walk in kept-row order, over the rows that move a count or carry a cue
        unsigned long long todo = __ballot(lane < nk && (s_in != s_out || ec >= 0));
        while (todo) {
            const int j = og_first(todo);
            todo &= todo - 1ull;
            const int sj = __builtin_amdgcn_readlane(s_in, j), so = __builtin_amdgcn_readlane(s_out, j);
            const int ej = __builtin_amdgcn_readlane(ec, j);
            if (sj != so) {
                cnt += (sj == lane ? 1 : 0) - (so == lane ? 1 : 0);
                voted = os_vote(cnt, top);
            }
            if (ej >= 0) {
                const int ok = voted == ej ? 1 : 0;
                voted_hit += ok;
                if (lane == ej) {
                    ++class_n;
                    class_hit += ok;
                }
            }
        }
        if (head + nk >= V) full = true;
        head = (head + nk) % V;
    }

    // ---- the class of the subset with the smallest voted recall class_hit / class_n, the smallest slot among equals
    unsigned long long have = __ballot(class_n > 0);
    const long long classes_scored = __popcll(have);
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
    const long long s[OS_SCORES] = {n_cue, hit, voted_hit, classes_scored, worst, worst_hit, worst_n};
#pragma unroll
    for (int i = 0; i < OS_SCORES; ++i)
        if (lane == i) out[i] = s[i];
    if (a.class_hits) a.class_hits[(size_t)g * 64 + lane] = class_hit;
}
