// Head fine-tuning (include/cpnative.h, cp_online_finetune_*): a user's projection (16 x 512 + 16) and class rows (K x 16) by
// gradient, on the tail inputs u the decoder's own encoder embeds once (cp_online_*tail_inputs, the enrol chains with fc7's
// output kept).  The f32 masters, their Adam moments, the initial values (the anchor), the T copy of W the forward multiplies
// by, the slots and the slabs live in a caller-owned state (OlfState in online_api.cuh).
//
// A step is two launches:
//   olf_step_kernel    one workgroup per chunk of OLF_CHUNK rows.  Per 16-row tile: z = W_T u + b through ol_tile, z^ as
//                      ol_tail_run forms it, the logits against E^ (normalised as ol_set_classes_kernel does, held in LDS) as
//                      ol_tail_tile sums them, the row softmax with one lane per class slot, g, dz^, dz; the tile's dz^T u goes
//                      onto the chunk's dW partial (16 x 512 f32 in registers: v_mfma_f32_16x16x4_f32 with u widened, so dz is
//                      never rounded to T), db, dE^ and the weighted loss onto theirs.  One slab store at the end.
//   olf_update_kernel  one thread per trained number: the slabs summed in chunk order in float64, the E^ -> E backward, the
//                      anchor term, Adam on the masters, the T copy of W for the next step, the step's loss.
// No floating-point atomics and no reduction whose order depends on the grid: a step's result depends on the inputs and
// OLF_CHUNK only.
#pragma once
#include "online_enroll.cuh"

constexpr int OLF_CHUNK = 64;                          // rows per workgroup of olf_step_kernel (CP_ONLINE_FINETUNE_CHUNK)
constexpr int OLF_W = CP_D_E * 512;                    // the trained numbers, in this order: W, b, E (64 rows, K used)
constexpr int OLF_B = OLF_W + CP_D_E;
constexpr int OLF_P = OLF_B + OL_MAXK * CP_D_E;
constexpr int OLF_SLAB = OLF_P + 16;                   // floats per slab: the partial gradients, then the weighted loss (float64)
constexpr int OLF_TRAIN_PROJ = 1, OLF_TRAIN_ROWS = 2;  // cp_online_finetune_steps flags
static_assert(OLF_CHUNK % 16 == 0 && OLF_P % 16 == 0 && OLF_SLAB % 32 == 0 && CP_D_E == 16, "slab layout");

struct OlfHead {                          // at the start of the state
    long long step;                       // Adam steps taken
    int n, K;
    int count[OL_MAXK];                   // windows per slot
    float wc[OL_MAXK];                    // w_i of a window of slot c
};

// cp_online_finetune_init: masters and their initial values, zero moments and gradient, the T copy of W, the slots, the
// per-slot counts and weights.  One workgroup.
struct OlfInitArgs {
    OlfHead* head;
    const float *W, *b, *E;               // (16,512), (16), (K,16)
    const int32_t* slots_in;
    float *theta, *theta0, *m, *v;
    void* wT;
    int32_t* slots;
    double* grad;
    int n, K, balanced;
};

template <typename T>
__global__ __launch_bounds__(1024) void olf_init_kernel(OlfInitArgs a) {
    __shared__ int cnt[OL_MAXK];
    const int tid = threadIdx.x;
    if (tid < OL_MAXK) cnt[tid] = 0;
    __syncthreads();
    for (int e = tid; e < OLF_P; e += 1024) {
        float v = 0.f;
        if (e < OLF_W) v = a.W[e];
        else if (e < OLF_B) v = a.b[e - OLF_W];
        else if (e - OLF_B < a.K * CP_D_E) v = a.E[e - OLF_B];
        a.theta[e] = v;
        a.theta0[e] = v;
        a.m[e] = 0.f;
        a.v[e] = 0.f;
        a.grad[e] = 0.0;
        if (e < OLF_W) ((T*)a.wT)[e] = ol_cvt<T>(v);
    }
    for (int i = tid; i < a.n; i += 1024) {
        const int s = a.slots_in[i];
        a.slots[i] = s;
        if (s >= 0 && s < a.K) atomicAdd(&cnt[s], 1);          // (integers: the order does not matter)
    }
    __syncthreads();
    if (tid < OL_MAXK) {
        int present = 0, total = 0;
        for (int c = 0; c < a.K; ++c) {
            present += cnt[c] > 0;
            total += cnt[c];
        }
        float w = 0.f;
        if (tid < a.K && cnt[tid] > 0)
            w = a.balanced ? (float)(1.0 / ((double)present * (double)cnt[tid])) : (float)(1.0 / (double)total);
        a.head->wc[tid] = w;
        a.head->count[tid] = tid < a.K ? cnt[tid] : 0;
    }
    if (tid == 0) {
        a.head->step = 0;
        a.head->n = a.n;
        a.head->K = a.K;
    }
}

struct OlfStepArgs {
    OlLayerArgs proj;         // act = u (N,512) in T, w = the T copy of W, bias = the master b
    OlfHead* head;
    const float* E;           // master rows (64,16)
    const int32_t* slots;     // [N]
    float* slabs;             // [chunks][OLF_SLAB]
    int N, K;
    float scale;
};

template <typename T>
struct OlfLds {
    OlTileLds<T> L;
    float en[OL_MAXK][17];    // E^
    float zn[16][17];         // z^ of the tile
    float dz[16][20];         // (stride 20: the two row groups of each half of the dW product's A read land 16 banks apart)
    float g[16][OL_MAXK + 1]; // the logits, then g
    float nrm[16];            // |z|
    float wrow[16];           // w_i
    int slot[16];             // < 0: the row takes no part (past N, or a slot outside 0..K-1)
    double loss[16];
};

template <typename T> __device__ __forceinline__ float olf_widen(T v);
template <> __device__ __forceinline__ float olf_widen<float>(float v) { return v; }
template <> __device__ __forceinline__ float olf_widen<bf16_t>(bf16_t v) { return bf2f(v); }

template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olf_step_kernel(OlfStepArgs a) {
#pragma clang fp contract(off)
    __shared__ OlfLds<T> S;
    OlTileLds<T>& L = S.L;
    constexpr int EPC = 16 / (int)sizeof(T), lda = 512 + EPC;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, h = lane >> 4;
    const int N = a.N, K = a.K;
    const int row_begin = blockIdx.x * OLF_CHUNK, row_end = min(N, row_begin + OLF_CHUNK);
    if (blockIdx.x == 0 && tid == 0) a.head->step += 1;        // this step's number, for the update kernel behind this launch
    if (tid < K) {                                             // as ol_set_classes_kernel
        float ss = 0.f;
        for (int d = 0; d < 16; ++d) ss += a.E[tid * 16 + d] * a.E[tid * 16 + d];
        const float n = sqrtf(ss);
        for (int d = 0; d < 16; ++d) S.en[tid][d] = a.E[tid * 16 + d] / n;
    }
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)a.proj.w, 512, 0, wf);
    // this wave's share of the chunk's dW: column blocks 4 wave .. 4 wave + 3, element r of a lane = dW[4 h + r][16 cb + r16]
    f32x4 dw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dw[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // thread (c, d) = (tid >> 4, tid & 15) and (32 + (tid >> 4), tid & 15) of dE^; thread d < 16 of db; thread 16 the loss
    const int ec0 = tid >> 4, ec1 = ec0 + OL_THREADS / 16, ed = tid & 15;
    float de0 = 0.f, de1 = 0.f, db = 0.f;
    double loss = 0.0;
    for (int m0 = row_begin; m0 < row_end; m0 += 16) {
        ol_tile<T, false>(a.proj, L, 512, 0, m0, N, wf);       // (its first barrier also puts en behind the writes above)
        if (tid < 16) {                                        // as ol_tail_tile: z, then z / sqrtf(ss), in f32
            float z[16], ss = 0.f;
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                z[d] = L.red[0][tid][d] + a.proj.bias[d];
                ss += z[d] * z[d];
            }
            const float nrm = sqrtf(ss);
#pragma unroll
            for (int d = 0; d < 16; ++d) S.zn[tid][d] = z[d] / nrm;
            S.nrm[tid] = nrm;
            int sl = -1;
            if (m0 + tid < row_end) {
                sl = a.slots[m0 + tid];
                if (sl < 0 || sl >= K) sl = -1;
            }
            S.slot[tid] = sl;
            S.wrow[tid] = sl >= 0 ? a.head->wc[sl] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < 16 * K; e += OL_THREADS) {       // the cosines as ol_tail_tile sums them, times scale
            const int row = e / K, k = e % K;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 16; ++d) s += S.zn[row][d] * S.en[k][d];
            S.g[row][k] = s * a.scale;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {                       // softmax of rows 2 wave, 2 wave + 1: lane c is class slot c
            const int row = wave * 2 + rr, sl = S.slot[row];
            const bool on = lane < K;
            const float l = on ? S.g[row][lane] : -INFINITY;
            float mx = l;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            const float ex = on ? expf(l - mx) : 0.f;
            float sum = ex;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            const float p = ex / sum, w = S.wrow[row];
            if (on) S.g[row][lane] = sl >= 0 ? w * a.scale * (p - (lane == sl ? 1.f : 0.f)) : 0.f;
            if (sl < 0) {
                if (lane == 0) S.loss[row] = 0.0;
            } else if (lane == sl) {
                S.loss[row] = (double)w * (double)(logf(sum) - (l - mx));
            }
        }
        __syncthreads();
        for (int r = 0; r < 16; ++r) {                         // dE^ += g^T z^, the tile's rows in order
            if (S.slot[r] < 0) continue;
            if (ec0 < K) de0 += S.g[r][ec0] * S.zn[r][ed];
            if (ec1 < K) de1 += S.g[r][ec1] * S.zn[r][ed];
        }
        if (tid < 256) {                                       // dz^ = g E^, dz = (dz^ - z^ (z^ . dz^)) / |z|
            const int row = tid >> 4, d = tid & 15;
            float s = 0.f;
            for (int c = 0; c < K; ++c) s += S.g[row][c] * S.en[c][d];
            float dot = S.zn[row][d] * s;
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
            const float v = (s - S.zn[row][d] * dot) / S.nrm[row];
            S.dz[row][d] = S.slot[row] >= 0 ? v : 0.f;
        }
        __syncthreads();
        if (tid < 16) {
            for (int r = 0; r < 16; ++r) db += S.dz[r][tid];
        } else if (tid == 16) {
            for (int r = 0; r < 16; ++r) loss += S.loss[r];
        }
        // dW += dz^T u: A = dz^T (lane: d = r16, row kg + 4 h), B = u widened (lane: row kg + 4 h, column 16 cb + r16).  A
        // 32-bit LDS read sees 32 banks and is served in two halves of 32 lanes.  With rows kg + 4 h and a row stride of
        // 512 + EPC the 16-lane groups h = 0, 1 of the first half (and h = 2, 3 of the second) start 16 banks apart and take 16
        // banks each: no conflict.  (Rows 4 kg + h would start the groups 4 banks apart: two lanes on twelve banks of each half.)
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
            const int row = kg + 4 * h;
            const float av = S.dz[row][r16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float bv = olf_widen<T>(L.a[row * lda + (wave * 4 + i) * 16 + r16]);
                dw[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, dw[i], 0, 0, 0);
            }
        }
        __syncthreads();                                       // L.a, zn, g, dz and slot are rewritten by the next tile
    }
    float* slab = a.slabs + (size_t)blockIdx.x * OLF_SLAB;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) slab[(4 * h + r) * 512 + (wave * 4 + i) * 16 + r16] = dw[i][r];
    slab[OLF_B + ec0 * 16 + ed] = de0;
    slab[OLF_B + ec1 * 16 + ed] = de1;
    if (tid < 16) slab[OLF_W + tid] = db;
    else if (tid == 16) *(double*)(slab + OLF_P) = loss;
}

struct OlfUpdateArgs {
    const OlfHead* head;
    float *theta, *m, *v;
    const float* theta0;
    void* wT;
    double* grad;             // [OLF_P] the step's reduced gradient
    const float* slabs;
    double* loss;             // this step's entry of loss_out
    int chunks, K, flags;
    double lr, lr_rows, anchor;
};

constexpr int OLF_UPDATE_THREADS = 64;    // one wave per workgroup: 145 workgroups, so that the slab reads spread over the chip

// grid OLF_P / 64 + 1, 64 threads: thread e < OLF_P owns trained number e, thread OLF_P the loss.  A 16-lane group is 16
// columns of a row of W, b, or one class row.  The sums add the slabs in chunk order; eight loads at a time are in flight.
template <typename T>
__global__ __launch_bounds__(OLF_UPDATE_THREADS) void olf_update_kernel(OlfUpdateArgs a) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * OLF_UPDATE_THREADS + threadIdx.x;
    const bool param = e < OLF_P, is_row = param && e >= OLF_B;
    const bool live = param && (!is_row || (e - OLF_B) / 16 < a.K);
    if (e == OLF_P) {
        double s = 0.0;
#pragma unroll 8
        for (int j = 0; j < a.chunks; ++j) s += *(const double*)(a.slabs + (size_t)j * OLF_SLAB + OLF_P);
        *a.loss = s;
    }
    double s = 0.0;
    if (live) {
#pragma unroll 8
        for (int j = 0; j < a.chunks; ++j) s += (double)a.slabs[(size_t)j * OLF_SLAB + e];
    }
    const float th = live ? a.theta[e] : 0.f;
    // class rows: E^ = E / |E| as ol_set_classes_kernel forms it, dE = (dE^ - E^ (E^ . dE^)) / |E|.  Every lane runs the
    // shuffles; what a lane outside the class rows computes here is not used
    const int base = threadIdx.x & 48;                        // first lane of this 16-lane group in its wave
    float ss = 0.f;
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const float x = __shfl(th, base + d, 64);
        ss += x * x;
    }
    const float len = sqrtf(ss);
    const double eh = (double)(th / len);
    double dot = eh * s;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (!live) return;
    double g = is_row ? (s - eh * dot) / (double)len : s;
    g += a.anchor * ((double)th - (double)a.theta0[e]);
    a.grad[e] = g;
    if (!(a.flags & (is_row ? OLF_TRAIN_ROWS : OLF_TRAIN_PROJ))) return;
    const double t = (double)a.head->step, b1 = 0.9, b2 = 0.999, eps = 1e-8;
    const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
    const float mn = (float)(b1 * (double)a.m[e] + (1.0 - b1) * g);
    const float vn = (float)(b2 * (double)a.v[e] + (1.0 - b2) * g * g);
    const double denom = sqrt((double)vn) / sqrt(bc2) + eps;
    const float pn = (float)((double)th - ((is_row ? a.lr_rows : a.lr) / bc1) * ((double)mn / denom));
    a.m[e] = mn;
    a.v[e] = vn;
    a.theta[e] = pn;
    if (e < OLF_W) ((T*)a.wT)[e] = ol_cvt<T>(pn);
}

// cp_online_*set_projection: W (16,512) f32 -> the tail's weights in T, b -> its bias
template <typename T>
__global__ __launch_bounds__(256) void olf_set_projection_kernel(const float* __restrict__ W, const float* __restrict__ b, T* __restrict__ Wd,
                                                                 float* __restrict__ bd) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < OLF_W) Wd[e] = ol_cvt<T>(W[e]);
    if (e < CP_D_E) bd[e] = b[e];
}

// cp_online_*projection: the tail's weights widened, and its bias
template <typename T>
__global__ __launch_bounds__(256) void olf_get_projection_kernel(const T* __restrict__ Wd, const float* __restrict__ bd, float* __restrict__ W,
                                                                 float* __restrict__ b) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < OLF_W) W[e] = olf_widen<T>(Wd[e]);
    if (e < CP_D_E) b[e] = bd[e];
}
