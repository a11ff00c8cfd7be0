// Multi-stream online decoding (include/cpnative.h, cp_online_multi_*): S <= 256 live sEMG streams share one model, one set of
// folded weights and one chain of ten launches per push, whatever S is.  Each stream keeps its own OlState (filter, RMS
// history, sample count, vote ring, class table); the rows of all streams run through the encoder together.
//
//   olm_frontend_kernel  grid S: workgroup s takes the prefix of the sample counts and of the windows they emit over streams
//                        0..s-1 (their n_seen before this push: nobody writes n_seen in this launch), runs ol_frontend_run on
//                        its samples and writes its windows from packed row row0; OlmMeta[s] keeps row0, M_s and n_seen after
//   olm_layer_kernel     conv2, fc1..fc7 over all R rows: grid (feature tiles [x 12 positions] x row blocks); each workgroup
//                        loads its weight slice into registers once and runs ol_layer_tiles over its 16-row tiles
//   olm_tail_kernel      grid S: workgroup s stores n_seen, then ol_tail_run over its M_s rows against its own class table
// The per-row arithmetic is that of csrc/online.cuh through the same device functions (ol_frontend_run, ol_tile,
// ol_layer_tiles, ol_tail_run): a row's values do not depend on the tile it falls in, so every stream's outputs are
// bit-identical to those of a single-stream decoder.  Every hand-off between workgroups is a launch boundary.
#pragma once
#include "online.cuh"

constexpr int OLM_MAXS = 256;            // streams (CP_ONLINE_MULTI_MAX_STREAMS)
constexpr int OLM_TARGET_WG = 512;       // workgroups an encoder launch aims for when there are rows enough

struct OlmMeta {                         // what the front end leaves for the tail, per stream
    long long n_seen;                    // samples seen after this push
    int row0, m;                         // first packed row and windows of this push
};

struct OlmFrontArgs {
    OlFrontArgs f;                       // raw: packed samples; X, windows: packed rows; map_src, map_fill: one row per stream
                                         // (f.st and f.n are unused)
    OlState* states;                     // [S]
    OlmMeta* meta;                       // [S]
    const int32_t* counts;               // [S] samples of each stream in this push
    long long total_samples;
    int rows, max_m;                     // rows of this push, windows one stream may emit
};

template <int NB>
__global__ __launch_bounds__(256) void olm_frontend_kernel(OlmFrontArgs p) {
    __shared__ float xs[OL_FRONT_PIECE * OL_C];
    __shared__ unsigned long long s_off;
    __shared__ int r_off;
    const int s = blockIdx.x, tid = threadIdx.x, phase = p.f.phase;
    if (tid == 0) {
        s_off = 0;
        r_off = 0;
    }
    __syncthreads();
    for (int j = tid; j < s; j += 256) {                 // integer sums: the order of the atomics does not matter
        const long long nj = p.counts[j] > 0 ? p.counts[j] : 0;
        const long long sj = p.states[j].n_seen;
        atomicAdd(&s_off, (unsigned long long)nj);
        atomicAdd(&r_off, (int)(ol_windows_before(sj + nj, phase) - ol_windows_before(sj, phase)));
    }
    __syncthreads();
    OlState* st = p.states + s;
    const long long n0 = st->n_seen, soff = (long long)s_off;
    const int row0 = r_off;
    long long n = p.counts[s];
    long long m = ol_windows_before(n0 + n, phase) - ol_windows_before(n0, phase);
    // counts that disagree with the totals the caller passed: the stream is left alone rather than read or written out of bounds
    if (n < 0 || soff + n > p.total_samples || row0 + m > p.rows || m > p.max_m) {
        n = 0;
        m = 0;
    }
    if (n > 0)
        ol_frontend_run<NB>(p.f, st, p.f.raw + soff * OL_C, n, n0, p.f.X + (size_t)row0 * OL_C,
                            p.f.windows ? p.f.windows + (size_t)row0 * OL_C : nullptr, xs, s);
    if (tid == 0) {
        p.meta[s].n_seen = n0 + n;
        p.meta[s].row0 = row0;
        p.meta[s].m = (int)m;
    }
}

struct OlmLayerArgs {
    OlLayerArgs l;                       // l.st is unused
    int rows, tiles_per_block;
};

// conv2 (CONV: grid 4 feature tiles x 12 positions x row blocks) or one fc layer (grid F/16 x row blocks)
template <typename T, bool CONV>
__global__ __launch_bounds__(OL_THREADS) void olm_layer_kernel(OlmLayerArgs a) {
    __shared__ OlTileLds<T> L;
    const int rb = CONV ? (int)blockIdx.z : (int)blockIdx.y;
    const int m_begin = rb * a.tiles_per_block * 16;
    if (m_begin >= a.rows) return;
    const int m_end = min(a.rows, m_begin + a.tiles_per_block * 16);
    ol_layer_tiles<T, CONV>(a.l, L, blockIdx.x * 16, CONV ? (int)blockIdx.y : 0, m_begin, m_end, a.rows);
}

struct OlmTailArgs {
    OlLayerArgs proj;                    // act = fc7 output of all rows, w / bias = folded projection
    OlState* states;
    const OlmMeta* meta;
    int vote;
    int32_t* pred;                       // [R] packed rows
    int32_t* voted;                      // [R]
    float* logits;                       // optional [R][OL_MAXK], columns >= K_s not written
    float* emb;                          // optional [R][16]: z / |z| of every packed row
};

template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olm_tail_kernel(OlmTailArgs t) {
    __shared__ OlTailLds<T> S;
    const int s = blockIdx.x;
    OlState* st = t.states + s;
    const OlmMeta mt = t.meta[s];
    if (threadIdx.x == 0) st->n_seen = mt.n_seen;
    if (mt.m <= 0) return;
    OlLayerArgs proj = t.proj;
    proj.act = (const T*)t.proj.act + (size_t)mt.row0 * 512;
    ol_tail_run<T>(proj, st, mt.m, t.vote, t.pred + mt.row0, t.voted + mt.row0,
                   t.logits ? t.logits + (size_t)mt.row0 * OL_MAXK : nullptr, OL_MAXK,
                   t.emb ? t.emb + (size_t)mt.row0 * 16 : nullptr, S);
}

// cp_online_multi_reset: the stream part of streams first .. first + gridDim.x - 1 to zero (as cp_online_reset's memset)
__global__ __launch_bounds__(256) void olm_reset_kernel(OlState* states, int first) {
    int* p = (int*)(states + first + blockIdx.x);
    for (int i = threadIdx.x; i < (int)(offsetof(OlState, K) / 4); i += 256) p[i] = 0;
}
