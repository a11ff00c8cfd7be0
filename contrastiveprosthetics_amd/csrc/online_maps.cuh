// Electrode-map sweep (include/cpnative.h, cp_online_*map_sweep): many electrode maps over one cued recording, each scored as a
// fresh stream of the decoder would decode the recording under that map.  `score_channel_maps` of
// contrastiveprosthetics_amd/online.py states the definition (set_channel_map, push, count); this pass reproduces its pred and
// voted exactly.
//
// The front end's channels are independent and a map only chooses which raw column a model channel filters, so the
// un-normalised RMS series R (M, 12) of the recording (cp_online_windows with mean 0 and std 1: (r - 0) / 1 == r) holds every
// value any map needs.  Rows are laid out g M + k (map g, window k) and run in chunks:
//   olmap_build_kernel   row (g, k): x[d] = src[d] >= 0 ? (R[k][src[d]] - mean[d]) / sd[d] : fill[d], the front end's own
//                        expression on the same operands (contraction off), with the front end's clamps
//   olm_layer_kernel     (csrc/online_multi.cuh) conv2, fc1..fc7 over the chunk: grid (feature tiles [x 12 positions] x row
//                        blocks), each workgroup ol_layer_tiles over its own whole 16-row tiles; a row's value does not depend
//                        on the tile, chunk or call it falls in.  The adaptive forms run their frozen chain (ola_conv_chain /
//                        ola_fc with OLA_FROZEN) in pieces of <= 256 rows instead
//   olmap_tail_kernel    ol_tail_tile per 16-row tile: projection, z / |z|, logits, first-maximum argmax -> the row's slot
// and, once every chunk is done,
//   olmap_vote_kernel    one wave per map walks its M slots in order through ol_vote_step from an empty ring, compares pred
//                        and voted with the cue and writes integer counters; the slots become class ids on the way out
#pragma once
#include "online_multi.cuh"

constexpr int OLMAP_SCORES = 3;          // CP_ONLINE_MAP_SCORES: rows, raw_hits, voted_hits
constexpr int OLMAP_WAVES = 4;           // maps per workgroup of olmap_vote_kernel

struct OlMapBuildArgs {
    const float* R;                      // [M][12] un-normalised RMS series
    const float* mean_std;               // [2][12]
    const int32_t* src;                  // [n_maps][12]
    const float* fill;                   // [n_maps][12]
    float* X;                            // [rows][12] the chunk's windows
    long long row0;                      // first row (g M + k) of the chunk
    int rows, M;
};

__global__ __launch_bounds__(256) void olmap_build_kernel(OlMapBuildArgs a) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)a.rows * OL_C) return;
    const int d = (int)(e % OL_C);
    const long long r = a.row0 + e / OL_C;
    const long long g = r / a.M, k = r % a.M;
    const int s = a.src[g * OL_C + d];
    float v;
    if (s < 0) {
        const float f = a.fill[g * OL_C + d];
        v = isfinite(f) ? f : 0.f;
    } else {
        const float rms = a.R[k * OL_C + (s < OL_C ? s : OL_C - 1)];
        v = (rms - a.mean_std[d]) / a.mean_std[OL_C + d];          // ol_frontend_run, emg_normalize_kernel
    }
    a.X[e] = v;
}

struct OlMapTailArgs {
    OlLayerArgs proj;                    // act = fc7 output of the chunk [rows][512]
    const OlState* st;                   // the class table
    int32_t* slot;                       // the chunk's part of pred: [rows] slots
    int rows, tiles_per_block;
};

template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olmap_tail_kernel(OlMapTailArgs a) {
    __shared__ OlTailLds<T> S;
    const int m_begin = blockIdx.x * a.tiles_per_block * 16;
    if (m_begin >= a.rows) return;
    const int m_end = min(a.rows, m_begin + a.tiles_per_block * 16);
    const int K = a.st->K;
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)a.proj.w, 512, 0, wf);
    for (int m0 = m_begin; m0 < m_end; m0 += 16) ol_tail_tile<T>(a.proj, a.st, K, m0, a.rows, nullptr, 0, nullptr, a.slot, S, wf);
}

struct OlMapVoteArgs {
    const OlState* st;                   // ids
    const int32_t* expected;             // [M] cue slot; outside 0..K-1: not scored
    int32_t* pred;                       // [n_maps][M] slots in, class ids out
    int32_t* voted;                      // optional [n_maps][M] class ids
    long long* scores;                   // [n_maps][OLMAP_SCORES]
    int32_t* class_hits;                 // optional [n_maps][64] voted hits per slot
    int n_maps, M, vote;
};

__global__ __launch_bounds__(64 * OLMAP_WAVES) void olmap_vote_kernel(OlMapVoteArgs a) {
    __shared__ int ring_all[OLMAP_WAVES][OL_MAXVOTE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * OLMAP_WAVES + wave;
    if (g >= a.n_maps) return;                             // (no workgroup barrier below: the waves do not meet)
    int* ring = ring_all[wave];
    const int V = a.vote, K = a.st->K;
    const int my_id = lane < K ? a.st->ids[lane] : 0;
    int32_t* pred = a.pred + (size_t)g * a.M;
    int32_t* voted = a.voted ? a.voted + (size_t)g * a.M : nullptr;
    int head = 0, len = 0, cnt = 0;                        // an empty ring
    long long rows = 0, raw_hits = 0, voted_hits = 0;
    int class_hit = 0;                                     // voted hits of slot `lane`
    for (int base = 0; base < a.M; base += 64) {
        const int nb = min(64, a.M - base);
        int pj_mine = 0, e_mine = -1, v_mine = 0;
        if (lane < nb) {
            pj_mine = pred[base + lane];
            pj_mine = pj_mine < 0 ? 0 : (pj_mine < K ? pj_mine : K - 1);       // (a slot the tail wrote: 0..K-1)
            e_mine = a.expected[base + lane];
            if (e_mine < 0 || e_mine >= K) e_mine = -1;
        }
        for (int j = 0; j < nb; ++j) {
            const int pj = __builtin_amdgcn_readlane(pj_mine, j), ej = __builtin_amdgcn_readlane(e_mine, j);
            const int vj = ol_vote_step(ring, head, len, cnt, V, pj, lane);
            if (lane == j) v_mine = vj;
            if (ej >= 0) {
                ++rows;
                raw_hits += pj == ej;
                voted_hits += vj == ej;
                if (lane == ej) class_hit += vj == ej;
            }
        }
        const int pid = __shfl(my_id, pj_mine, 64), vid = __shfl(my_id, v_mine, 64);      // (every lane takes part)
        if (lane < nb) {
            pred[base + lane] = pid;
            if (voted) voted[base + lane] = vid;
        }
    }
    const long long s[OLMAP_SCORES] = {rows, raw_hits, voted_hits};
#pragma unroll
    for (int i = 0; i < OLMAP_SCORES; ++i)
        if (lane == i) a.scores[(size_t)g * OLMAP_SCORES + i] = s[i];
    if (a.class_hits) a.class_hits[(size_t)g * 64 + lane] = class_hit;
}
