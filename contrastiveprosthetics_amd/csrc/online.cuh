// Online grasp decoding (include/cpnative.h, cp_online_*): consecutive chunks of a live 2 kHz, 12-channel sEMG stream ->
// one predicted and one voted class per 10 ms window.  Everything a stream carries from one push to the next -- IIR state,
// RMS history, sample count, vote ring, class table, folded weights -- lives in the caller's workspace (OlState and the
// carve of ol_carve in online_api.cuh); nothing is process-global.
//
// A push is a chain of ten launches on one stream:
//   ol_frontend_kernel   one workgroup; 12 threads run the float64 recurrences of preprocess_kernel (csrc/preprocess.cuh)
//                        from the stored state, round at the same points, normalise, and write the windows the chunk
//                        completes; the window count M goes into the state for the launches behind it
//   ol_layer_kernel      conv1 + conv2 (BN1 folded, position-dependent shift), then fc1..fc7 (BN2..BN8 folded): each
//                        workgroup owns 16 output features (and, for conv2, one of the 12 positions) and streams its weight
//                        slice into registers once; its 8 waves split K in chunks of 32 and the partial tiles are summed in a
//                        fixed order, so a row's result depends neither on M nor on the chunking
//   ol_tail_kernel       projection (BN8 folded), L2 normalisation, logits against the class table, argmax and the vote ring
// Windows are padded to 16-row tiles (v_mfma_f32_16x16x32_bf16, or four v_mfma_f32_16x16x4_f32 per 16 k for f32); rows past
// M are staged as zeros and never stored.
#pragma once
#include "common.cuh"

constexpr int OL_C = 12;                 // channels
constexpr int OL_NW = 8;                 // waves per workgroup of the encoder launches
constexpr int OL_THREADS = OL_NW * 64;
constexpr int OL_KC = 32;                // k per chunk (one bf16 MFMA, four f32 ones per 16 k)
constexpr int OL_MAXCH = 3;              // chunks per wave: K <= 768 = 3 x 8 x 32
constexpr int OL_KMAX = 768;
constexpr int OL_CONV_K = 192;           // conv2: 3 taps x 64 input channels per output position
constexpr int OL_MAXK = 64;              // classes
constexpr int OL_MAXVOTE = 256;
constexpr int OL_MAXM = 256;             // windows per push (CP_ONLINE_MAX_WINDOWS)
constexpr int OL_MAXCOEF = 17;
constexpr int OL_RMS = 11;               // RMS window (code/constants.py:68)
constexpr int OL_STRIDE = 20;            // 2 kHz -> 100 Hz
constexpr int OL_FRONT_PIECE = 1024;     // samples staged in LDS per step of the front end

// Per-stream state at the start of the workspace.  Everything before `K` is the stream part that cp_online_reset zeroes;
// the class part survives a reset.
struct OlState {
    double z[OL_C][OL_MAXCOEF - 1];      // direct form II transposed state, float64
    double tmp[OL_C];                    // running float64 sum of squares
    float ring[OL_C][OL_RMS + 1];        // squares of the last 12 samples (ring[c][k] = k samples ago)
    float sq0[OL_C];                     // square of sample 0 (the 'nearest' edge extension)
    long long n_seen;                    // raw samples consumed
    int m_cur;                           // windows emitted by the current push
    int vote_head, vote_len;
    int pad0;
    int vote_ring[OL_MAXVOTE];           // class indices (into the sorted table)
    int K;                               // ---- class part
    int pad1[3];
    int ids[OL_MAXK];                    // class id of each table row, ascending
    float table[OL_MAXK][16];            // L2-normalised class embeddings
};

struct OlFrontArgs {
    const float* raw;                    // [n][12]
    long long n;
    OlState* st;
    float* X;                            // [max windows][12] normalised windows
    float* windows;                      // optional copy for the caller
    const float* mean_std;               // [2][12]
    const int32_t* map_src;              // optional electrode map [streams][12]: the raw column of each model channel, < 0: masked
    const float* map_fill;               // [streams][12]: what a masked channel emits (NULL with map_src == NULL: the identity)
    int n_coef, phase;
    float gain;
    double b[OL_MAXCOEF], a[OL_MAXCOEF]; // normalised (a[0] == 1)
};

// Windows final once N raw samples have arrived (include/cpnative.h: c(N))
__device__ __forceinline__ long long ol_windows_before(long long N, int phase) {
    const long long v = (N - phase + 9) / OL_STRIDE;
    return v > 0 ? v : 0;
}

// The recurrences of preprocess_kernel<NB, 11> carried across calls: same operations, same order, same rounding points,
// floating-point contraction off.  Window k is the RMS-series position phase + 20 k, i.e. raw sample phase + 20 k + 10.
// One workgroup of 256 threads runs one stream: n samples of raw from the stream's state st (n0 samples seen so far), the
// windows to X and windows (if not NULL) from row 0.  Updates the filter and RMS state, not n_seen; returns the number
// of windows on thread 0.  Behind a barrier on return.
// Electrode map (row map_row of p.map_src / p.map_fill; none: the identity): thread c is model channel c.  It filters raw
// column src[c], keeps that filter's state in its own slots of st, normalises with its own mean and std and writes column c.
// A masked channel (src < 0) runs the recurrences on input 0 and emits fill[c] in every window.  The map is read once, in
// front of the sample loop; a value the host could not see is clamped here: src above 11 reads column 11, a fill that is
// not finite reads as 0.
template <int NB>
__device__ __forceinline__ int ol_frontend_run(const OlFrontArgs& p, OlState* st, const float* raw, long long n, long long n0,
                                               float* X, float* windows, float* xs, int map_row = 0) {
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    const bool on = c < OL_C;
    const int nb = NB > 0 ? NB : p.n_coef;
    constexpr int ZN = NB > 0 ? NB - 1 : OL_MAXCOEF - 1;
    constexpr int win = OL_RMS, half = win / 2, lead = win - 1 - half;
    const double dwin = (double)win;
    double z[ZN];
    float ring[win + 1];
    double tmp = 0.0;
    float sq0 = 0.f, mean = 0.f, sd = 1.f;
#pragma unroll
    for (int i = 0; i < ZN; ++i) z[i] = on ? st->z[c][i] : 0.0;
#pragma unroll
    for (int i = 0; i <= win; ++i) ring[i] = on ? st->ring[c][i] : 0.f;
    if (on) {
        tmp = st->tmp[c];
        sq0 = st->sq0[c];
        mean = p.mean_std[c];
        sd = p.mean_std[OL_C + c];
    }
    int col = on ? c : 0;                                  // raw column of this model channel
    bool masked = false;
    float fill = 0.f;
    if (on && p.map_src) {
        const int s = p.map_src[map_row * OL_C + c];
        masked = s < 0;
        col = masked ? c : (s < OL_C ? s : OL_C - 1);
        const float f = p.map_fill[map_row * OL_C + c];
        fill = isfinite(f) ? f : 0.f;
    }
    int j = 0;
    for (long long base = 0; base < n; base += OL_FRONT_PIECE) {
        const int len = (int)((n - base) < OL_FRONT_PIECE ? (n - base) : OL_FRONT_PIECE);
        __syncthreads();
        for (int e = threadIdx.x; e < len * OL_C; e += 256) xs[e] = raw[base * OL_C + e];
        __syncthreads();
        if (!on) continue;
        for (int tl = 0; tl < len; ++tl) {
            const long long t = n0 + base + tl;
            const float xin = masked ? 0.f : xs[tl * OL_C + col] * p.gain;
            const double xt = (double)xin;
            const double y = z[0] + p.b[0] * xt;
#pragma unroll
            for (int i = 0; i < ZN - 1; ++i)
                if (i < nb - 2) z[i] = (z[i + 1] + xt * p.b[i + 1]) - y * p.a[i + 1];
            z[nb - 2] = xt * p.b[nb - 1] - y * p.a[nb - 1];
            const float y32 = (float)y;
            const float sq = y32 * y32;
#pragma unroll
            for (int i = win; i > 0; --i) ring[i] = ring[i - 1];
            ring[0] = sq;
            if (t == 0) sq0 = sq;
            if (t <= lead) {
                if (t == 0) {
                    for (int k = 0; k <= half; ++k) tmp += (double)sq;
                } else {
                    tmp += (double)sq;
                }
            } else {
                const long long l = t - lead;
                const long long back = l - 1 - half;
                const float leaving = back <= 0 ? sq0 : ring[win];
                tmp += (double)sq - (double)leaving;
                const long long i = l - half;
                if (i >= p.phase && (i - p.phase) % OL_STRIDE == 0) {
                    const float r = sqrtf((float)(tmp / dwin));
                    const float v = masked ? fill : (r - mean) / sd;  // emg_normalize_kernel
                    X[j * OL_C + c] = v;
                    if (windows) windows[j * OL_C + c] = v;
                    ++j;
                }
            }
        }
    }
    if (on) {
#pragma unroll
        for (int i = 0; i < ZN; ++i) st->z[c][i] = z[i];
#pragma unroll
        for (int i = 0; i <= win; ++i) st->ring[c][i] = ring[i];
        st->tmp[c] = tmp;
        st->sq0[c] = sq0;
    }
    __syncthreads();
    return j;
}

template <int NB>
__global__ __launch_bounds__(256) void ol_frontend_kernel(OlFrontArgs p) {
    __shared__ float xs[OL_FRONT_PIECE * OL_C];
    OlState* st = p.st;
    const long long n0 = st->n_seen;
    const int j = ol_frontend_run<NB>(p, st, p.raw, p.n, n0, p.X, p.windows, xs);     // (every thread has read n_seen)
    if (threadIdx.x == 0) {
        st->n_seen = n0 + p.n;
        st->m_cur = j;
    }
}

struct OlLayerArgs {
    const void* act;          // [rows][K] input activations (fc layers)
    const float* x;           // conv: normalised windows [rows][12]
    const float* c1w;         // conv: conv1 taps [64][3]
    const float* c1b;         // conv: conv1 bias [64]
    const void* w;            // folded weights [F][K], compute dtype
    const float* bias;        // folded bias [positions][F]
    void* out;                // [rows][ldo], output feature pos * out_pos + f
    const OlState* st;
    int K, F, ldo, out_pos;
};

template <typename T> __device__ __forceinline__ T ol_cvt(float v);
template <> __device__ __forceinline__ float ol_cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t ol_cvt<bf16_t>(float v) { return f2bf(v); }

template <typename T> __device__ __forceinline__ void ol_mma(const uint4& a, const uint4& b, f32x4& acc);
template <> __device__ __forceinline__ void ol_mma<bf16_t>(const uint4& a, const uint4& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), acc, 0, 0, 0);
}
template <> __device__ __forceinline__ void ol_mma<float>(const uint4& a, const uint4& b, f32x4& acc) {
    // element e of lane group h = k 4h + e of this 16-k group, in both operands
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

// LDS of one 16-row tile: the A operand (rows padded by 16 bytes against bank conflicts) and the per-wave partial sums
template <typename T>
struct OlTileLds {
    static constexpr int EPC = 16 / (int)sizeof(T);
    T a[16 * (OL_KMAX + EPC)];
    float red[OL_NW][16][17];
};

// Weight fragments of this wave for features f0..f0+15: chunk i of the wave is chunk wave + 8 i of K.
template <typename T>
__device__ __forceinline__ void ol_load_weights(const T* __restrict__ W, int K, int f0, uint4 (&wf)[OL_MAXCH][OL_KC * (int)sizeof(T) / 64]) {
    constexpr int EPC = 16 / (int)sizeof(T), G = OL_KC / (4 * EPC);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, h = lane >> 4;
    const T* row = W + (size_t)(f0 + r16) * K;
#pragma unroll
    for (int i = 0; i < OL_MAXCH; ++i) {
        const int c = wave + i * OL_NW;
#pragma unroll
        for (int g = 0; g < G; ++g)
            wf[i][g] = c * OL_KC < K ? *(const uint4*)(row + c * OL_KC + g * 4 * EPC + h * EPC) : make_uint4(0, 0, 0, 0);
    }
}

// One 16-row tile: stage A (conv: compute conv1 for the three input positions of `pos`), multiply, and leave the summed
// 16 x 16 pre-activation tile in red[0] (rows = windows, columns = features f0..f0+15).  Ends behind a barrier.
template <typename T, bool CONV>
__device__ __forceinline__ void ol_tile(const OlLayerArgs& a, OlTileLds<T>& L, int K, int pos, int m0, int M,
                                        const uint4 (&wf)[OL_MAXCH][OL_KC * (int)sizeof(T) / 64]) {
#pragma clang fp contract(off)
    constexpr int EPC = 16 / (int)sizeof(T), G = OL_KC / (4 * EPC);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, h = lane >> 4;
    const int lda = K + EPC;
    if constexpr (CONV) {
        for (int e = tid; e < 16 * OL_CONV_K; e += OL_THREADS) {
            const int row = e / OL_CONV_K, k = e % OL_CONV_K, kw = k >> 6, ci = k & 63, q = pos + kw - 1;
            float v = 0.f;
            if (m0 + row < M && q >= 0 && q < OL_C) {
                const float* xr = a.x + (size_t)(m0 + row) * OL_C;
                float s = a.c1b[ci];
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int u = q + t - 1;
                    if (u >= 0 && u < OL_C) s = fmaf(a.c1w[ci * 3 + t], xr[u], s);
                }
                v = fmaxf(s, 0.f);
            }
            L.a[row * lda + k] = ol_cvt<T>(v);
        }
    } else {
        const int vpr = K / EPC;
        for (int e = tid; e < 16 * vpr; e += OL_THREADS) {
            const int row = e / vpr, v = e % vpr;
            uint4 d = make_uint4(0, 0, 0, 0);
            if (m0 + row < M) d = *((const uint4*)((const T*)a.act + (size_t)(m0 + row) * K) + v);
            *(uint4*)(L.a + row * lda + v * EPC) = d;
        }
    }
    __syncthreads();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < OL_MAXCH; ++i) {
        const int c = wave + i * OL_NW;
        if (c * OL_KC < K) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint4 av = *(const uint4*)(L.a + r16 * lda + c * OL_KC + g * 4 * EPC + h * EPC);
                ol_mma<T>(av, wf[i][g], acc);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) L.red[wave][h * 4 + r][r16] = acc[r];
    __syncthreads();
    if (tid < 256) {                                  // waves summed in a fixed order
        const int row = tid >> 4, col = tid & 15;
        float s = L.red[0][row][col];
#pragma unroll
        for (int w = 1; w < OL_NW; ++w) s += L.red[w][row][col];
        L.red[0][row][col] = s;                       // (each thread reads and writes only its own element)
    }
    __syncthreads();
}

// Tiles m_begin, m_begin + 16, .. < m_end of M rows for features f0..f0+15 (and position pos): out = relu(A W'^T + b')
template <typename T, bool CONV>
__device__ __forceinline__ void ol_layer_tiles(const OlLayerArgs& a, OlTileLds<T>& L, int f0, int pos, int m_begin, int m_end, int M) {
#pragma clang fp contract(off)
    const int K = CONV ? OL_CONV_K : a.K;
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)a.w, K, f0, wf);
    const int tid = threadIdx.x;
    for (int m0 = m_begin; m0 < m_end; m0 += 16) {
        ol_tile<T, CONV>(a, L, K, pos, m0, M, wf);
        if (tid < 256) {
            const int row = tid >> 4, col = tid & 15;
            if (m0 + row < M) {
                const float v = fmaxf(L.red[0][row][col] + a.bias[pos * a.F + f0 + col], 0.f);
                ((T*)a.out)[(size_t)(m0 + row) * a.ldo + pos * a.out_pos + f0 + col] = ol_cvt<T>(v);
            }
        }
        // the next tile's staging writes only L.a, which every wave finished reading before ol_tile's second barrier
    }
}

// conv2 (CONV: grid 4 feature tiles x 12 positions, conv1 recomputed from the windows) or one fc layer (grid F/16):
// out = relu(A W'^T + b') in the compute dtype
template <typename T, bool CONV>
__global__ __launch_bounds__(OL_THREADS) void ol_layer_kernel(OlLayerArgs a) {
    __shared__ OlTileLds<T> L;
    const int M = a.st->m_cur;
    if (M <= 0) return;
    ol_layer_tiles<T, CONV>(a, L, blockIdx.x * 16, CONV ? (int)blockIdx.y : 0, 0, M, M);
}

struct OlTailArgs {
    OlLayerArgs proj;         // act = fc7 output, w / bias = folded projection
    OlState* st;
    int vote;
    int32_t* pred;            // [M] class ids
    int32_t* voted;           // [M]
    float* logits;            // optional [M][K]
    float* emb;               // optional [M][16]: z / |z| of every window
};

// LDS of the tail
template <typename T>
struct OlTailLds {
    OlTileLds<T> L;
    float zn[16][17];
    float lg[16][OL_MAXK + 1];
    int pidx[OL_MAXM];
    int ring[OL_MAXVOTE];
};

// One 16-row tile of the tail, rows m0..m0+15 of the M rows of proj.act: projection -> z, z / |z|, logits against the table,
// argmax (first maximum).  Row j's slot (its index into the sorted table) goes to pidx[j], in LDS or in global memory, its
// logits to logits[j * ldl ..] (columns 0..K-1) if logits is given, its z / |z| to emb[j * 16 ..] if emb is given.  wf: the
// projection's fragments (ol_load_weights).  Ends behind a barrier.
template <typename T>
__device__ __forceinline__ void ol_tail_tile(const OlLayerArgs& proj, const OlState* st, int K, int m0, int M, float* logits, int ldl,
                                             float* emb, int* pidx, OlTailLds<T>& S,
                                             const uint4 (&wf)[OL_MAXCH][OL_KC * (int)sizeof(T) / 64]) {
#pragma clang fp contract(off)
    OlTileLds<T>& L = S.L;
    auto& zn = S.zn;
    auto& lg = S.lg;
    const int tid = threadIdx.x;
    ol_tile<T, false>(proj, L, 512, 0, m0, M, wf);
    if (tid < 16) {
        float z[16], ss = 0.f;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            z[d] = L.red[0][tid][d] + proj.bias[d];
            ss += z[d] * z[d];
        }
        const float nrm = sqrtf(ss);
#pragma unroll
        for (int d = 0; d < 16; ++d) zn[tid][d] = z[d] / nrm;
        if (emb && m0 + tid < M) {
#pragma unroll
            for (int d = 0; d < 16; ++d) emb[(size_t)(m0 + tid) * 16 + d] = zn[tid][d];
        }
    }
    __syncthreads();
    for (int e = tid; e < 16 * K; e += OL_THREADS) {
        const int row = e / K, k = e % K;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 16; ++d) s += zn[row][d] * st->table[k][d];
        lg[row][k] = s;
        if (logits && m0 + row < M) logits[(size_t)(m0 + row) * ldl + k] = s;
    }
    __syncthreads();
    if (tid < 16 && m0 + tid < M) {
        int best = 0;
        float bv = lg[tid][0];
        for (int k = 1; k < K; ++k)
            if (lg[tid][k] > bv) { bv = lg[tid][k]; best = k; }
        pidx[m0 + tid] = best;
    }
    __syncthreads();
}

// The vote ring, one wave: lane k keeps the count of slot k over the ring (cnt).  Slot pj enters at `head`, the oldest entry
// leaves once V are in; returns the slot with the most entries, the smallest among equals, on every lane.
__device__ __forceinline__ int ol_vote_step(int* ring, int& head, int& len, int& cnt, int V, int pj, int lane) {
    if (len == V) cnt -= ring[head] == lane;
    else ++len;
    cnt += pj == lane;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) ring[head] = pj;
    head = head + 1 == V ? 0 : head + 1;
    int key = (cnt << 8) | (255 - lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
    return 255 - (key & 255);
}

// ol_tail_tile over the M (1..OL_MAXM) rows of proj.act, then one wave runs the vote ring over the push's windows in order:
// mode of the last `vote` predictions, ties to the smallest class id (the table is sorted by id).
// Row j's outputs go to pred[j], voted[j], logits[j * ldl ..] (columns 0..K-1) and emb[j * 16 ..] (logits, emb: optional).
template <typename T>
__device__ __forceinline__ void ol_tail_run(const OlLayerArgs& proj, OlState* st, int M, int vote, int32_t* pred, int32_t* voted,
                                            float* logits, int ldl, float* emb, OlTailLds<T>& S) {
    auto& pidx = S.pidx;
    auto& ring = S.ring;
    const int K = st->K;
    const int tid = threadIdx.x;
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)proj.w, 512, 0, wf);
    for (int m0 = 0; m0 < M; m0 += 16) ol_tail_tile<T>(proj, st, K, m0, M, logits, ldl, emb, pidx, S, wf);
    if (tid < 64) {
        const int lane = tid, V = vote;
        int head = st->vote_head, len = st->vote_len;
        for (int i = lane; i < V; i += 64) ring[i] = st->vote_ring[i];
        __builtin_amdgcn_wave_barrier();
        int cnt = 0;
        for (int i = 0; i < len; ++i) cnt += ring[(head + V - len + i) % V] == lane;
        for (int j = 0; j < M; ++j) {
            const int pj = pidx[j];
            const int vj = ol_vote_step(ring, head, len, cnt, V, pj, lane);
            if (lane == 0) {
                pred[j] = st->ids[pj];
                voted[j] = st->ids[vj];
            }
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < V; i += 64) st->vote_ring[i] = ring[i];
        if (lane == 0) {
            st->vote_head = head;
            st->vote_len = len;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(OL_THREADS) void ol_tail_kernel(OlTailArgs t) {
    __shared__ OlTailLds<T> S;
    OlState* st = t.st;
    const int M = st->m_cur;
    if (M <= 0) return;
    ol_tail_run<T>(t.proj, st, M, t.vote, t.pred, t.voted, t.logits, st->K, t.emb, S);
}

// ---- cp_online_prepare: fold running-statistics BatchNorm into the layer behind it ------------------------------------
// BN(r) = s r + h with s = gamma / sqrt(var + eps), h = beta - mean s;  W (s r + h) + b = (W diag s) r + (b + W h).
struct OlFoldArgs {
    const float* W;           // source weight (row-major as the state_dict holds it)
    const float* b;           // source bias (NULL: none -- the projection)
    const float *g, *beta, *mean, *var;     // the BatchNorm in front of the layer
    float eps;
    void* Wd;                 // folded weight [F][K] in the compute dtype
    float* bd;                // folded bias [F] (mode 2: [12][64])
    int K;                    // destination row length
    int mode;                 // 0: plain, 1: fc1 (columns o*12+w -> w*64+o), 2: conv2 (taps [o][i][1][kw] -> [o][kw*64+i])
    const float* c1w_src;     // mode 2: conv1 copied as [64][3] + bias
    const float* c1b_src;
    float* c1w;
    float* c1b;
};

template <typename T>
__global__ __launch_bounds__(256) void ol_fold_kernel(OlFoldArgs a) {
#pragma clang fp contract(off)
    __shared__ float part[3][4];
    const int f = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;   // W h, split by tap for conv2
    for (int k = tid; k < a.K; k += 256) {
        int src, ch, tap = 0;
        if (a.mode == 0) { src = k; ch = k; }
        else if (a.mode == 1) { const int w = k >> 6, o = k & 63; src = o * 12 + w; ch = o; }
        else { tap = k >> 6; ch = k & 63; src = ch * 9 + 3 + tap; }
        const float s = a.g[ch] / sqrtf(a.var[ch] + a.eps);
        const float h = a.beta[ch] - a.mean[ch] * s;
        const float w = a.W[(size_t)f * (a.mode == 2 ? 576 : a.K) + src];
        ((T*)a.Wd)[(size_t)f * a.K + k] = ol_cvt<T>(w * s);
        if (tap == 0) acc0 += w * h;
        else if (tap == 1) acc1 += w * h;
        else acc2 += w * h;
    }
    const float v0 = wave_sum(acc0), v1 = wave_sum(acc1), v2 = wave_sum(acc2);
    if (lane == 0) { part[0][wave] = v0; part[1][wave] = v1; part[2][wave] = v2; }
    __syncthreads();
    if (tid == 0) {
        float sum[3];
        for (int i = 0; i < 3; ++i) sum[i] = ((part[i][0] + part[i][1]) + part[i][2]) + part[i][3];
        const float b0 = a.b ? a.b[f] : 0.f;
        if (a.mode != 2) {
            a.bd[f] = b0 + sum[0];
        } else {                                  // zero padding: the shift reaches an edge position through two taps only
            for (int w = 0; w < OL_C; ++w) {
                float v = b0;
                if (w > 0) v += sum[0];
                v += sum[1];
                if (w < OL_C - 1) v += sum[2];
                a.bd[w * 64 + f] = v;
            }
        }
    }
    if (a.mode == 2 && tid < 3) {
        a.c1w[f * 3 + tid] = a.c1w_src[f * 9 + 3 + tid];
        if (tid == 0) a.c1b[f] = a.c1b_src[f];
    }
}

// cp_online_set_classes: rows / |row|, ids, an empty vote ring
__global__ __launch_bounds__(64) void ol_set_classes_kernel(OlState* st, const float* __restrict__ table, const int32_t* __restrict__ ids, int K) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    if (k < K) {
        float ss = 0.f;
        for (int d = 0; d < 16; ++d) ss += table[k * 16 + d] * table[k * 16 + d];
        const float n = sqrtf(ss);
        for (int d = 0; d < 16; ++d) st->table[k][d] = table[k * 16 + d] / n;
        st->ids[k] = ids[k];
    }
    if (k == 0) {
        st->K = K;
        st->vote_head = 0;
        st->vote_len = 0;
    }
}
