// Per-stream projections of the multi-stream decoders (include/cpnative.h, cp_online_projections_* and the *_proj entries): a
// bank of one slot per stream, in a caller-owned buffer of its own next to the decoder workspace (whose layout does not change).
//
// Slot s of a bank in compute type T, olp_slot_bytes<T>() = 16 * 512 * sizeof(T) + 256 bytes from s * olp_slot_bytes<T>():
//   W    [16][512] T   exactly what olf_set_projection_kernel<T> writes into the workspace's pw (the same ol_cvt rounding)
//   b    [16] f32      directly behind W
//   set  one word      64 bytes behind W; 0: the stream has no projection of its own
// A zeroed bank therefore holds no projection.  A stream whose slot is not set reads the workspace's own projection, and the
// choice is made on the device from the set word, uniformly per workgroup (the tail) or per launch (enrolment, map sweep): a
// re-prepare of the workspace needs no bank work, a user's projection survives it, and an unset stream's outputs are what
// the kernels without a bank give, in every bit.
//
//   olp_set_kernel         one slot from f32 W (16,512), b (16); olp_get_kernel reads it back widened, with its set word
//   olp_clear_kernel       the set words of slots first .. first + gridDim.x - 1 to 0
//   olp_tail_kernel        olm_tail_kernel with workgroup s taking slot s
//   olp_accumulate_kernel  ole_accumulate_kernel with one slot
//   olp_map_tail_kernel    olmap_tail_kernel with one slot
// The three take the argument structs of the kernels they stand beside and run the same device functions (ol_tail_run,
// ol_tail_tile, ol_tile, ol_load_weights) on arguments whose w / bias point into the slot: a row's values are those of a
// single-stream decoder with the same projection installed.  The kernels they stand beside are launched as before by every
// entry that takes no bank.
#pragma once
#include "online_maps.cuh"
#include "online_finetune.cuh"

constexpr int OLP_SLOT_TAIL = 256;       // b (64 bytes), the set word, padding: every slot starts 256-aligned

template <typename T>
__host__ __device__ constexpr size_t olp_slot_bytes() {
    return (size_t)OLF_W * sizeof(T) + OLP_SLOT_TAIL;
}

struct OlpSlot {                         // one slot, or (tail) slot 0 of a bank
    const void* w;                       // [16][512] compute dtype
    const float* bias;                   // [16]
    const unsigned* set;
};

// slot s of the bank whose slot 0 is b
template <typename T>
__host__ __device__ __forceinline__ OlpSlot olp_slot(const OlpSlot& b, int s) {
    const size_t o = (size_t)s * olp_slot_bytes<T>();
    return OlpSlot{(const unsigned char*)b.w + o, (const float*)((const unsigned char*)b.bias + o),
                   (const unsigned*)((const unsigned char*)b.set + o)};
}

// proj with the slot's projection if the slot is set (the same answer in every thread of the launch that reads this slot)
__device__ __forceinline__ OlLayerArgs olp_choose(OlLayerArgs proj, const OlpSlot& sl) {
    if (*sl.set != 0u) {
        proj.w = sl.w;
        proj.bias = sl.bias;
    }
    return proj;
}

// cp_online_projections_set: olf_set_projection_kernel's stores into the slot, and the set word
template <typename T>
__global__ __launch_bounds__(256) void olp_set_kernel(const float* __restrict__ W, const float* __restrict__ b, T* __restrict__ Wd,
                                                      float* __restrict__ bd, unsigned* __restrict__ set) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < OLF_W) Wd[e] = ol_cvt<T>(W[e]);
    if (e < CP_D_E) bd[e] = b[e];
    if (e == 0) *set = 1u;
}

// cp_online_projections_get: the slot widened, and whether it is set (is_set optional)
template <typename T>
__global__ __launch_bounds__(256) void olp_get_kernel(OlpSlot sl, float* __restrict__ W, float* __restrict__ b, int32_t* __restrict__ is_set) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < OLF_W) W[e] = olf_widen<T>(((const T*)sl.w)[e]);
    if (e < CP_D_E) b[e] = sl.bias[e];
    if (e == 0 && is_set) *is_set = *sl.set != 0u ? 1 : 0;
}

// cp_online_projections_clear: set words `stride` bytes apart, one per workgroup
__global__ __launch_bounds__(64) void olp_clear_kernel(unsigned char* first_set, size_t stride) {
    if (threadIdx.x == 0) *(unsigned*)(first_set + (size_t)blockIdx.x * stride) = 0u;
}

// olm_tail_kernel (csrc/online_multi.cuh) with workgroup s reading slot s of the bank
template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olp_tail_kernel(OlmTailArgs t, OlpSlot bank) {
    __shared__ OlTailLds<T> S;
    const int s = blockIdx.x;
    OlState* st = t.states + s;
    const OlmMeta mt = t.meta[s];
    if (threadIdx.x == 0) st->n_seen = mt.n_seen;
    if (mt.m <= 0) return;
    OlLayerArgs proj = olp_choose(t.proj, olp_slot<T>(bank, s));
    proj.act = (const T*)t.proj.act + (size_t)mt.row0 * 512;
    ol_tail_run<T>(proj, st, mt.m, t.vote, t.pred + mt.row0, t.voted + mt.row0,
                   t.logits ? t.logits + (size_t)mt.row0 * OL_MAXK : nullptr, OL_MAXK,
                   t.emb ? t.emb + (size_t)mt.row0 * 16 : nullptr, S);
}

// olmap_tail_kernel (csrc/online_maps.cuh) with the projection of one slot
template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olp_map_tail_kernel(OlMapTailArgs a, OlpSlot sl) {
    __shared__ OlTailLds<T> S;
    const int m_begin = blockIdx.x * a.tiles_per_block * 16;
    if (m_begin >= a.rows) return;
    const int m_end = min(a.rows, m_begin + a.tiles_per_block * 16);
    const int K = a.st->K;
    const OlLayerArgs proj = olp_choose(a.proj, sl);
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)proj.w, 512, 0, wf);
    for (int m0 = m_begin; m0 < m_end; m0 += 16) ol_tail_tile<T>(proj, a.st, K, m0, a.rows, nullptr, 0, nullptr, a.slot, S, wf);
}

// ole_accumulate_kernel (csrc/online_enroll.cuh) with the projection of one slot: the same statements in the same order on
// proj instead of a.proj
template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olp_accumulate_kernel(OleAccArgs a, OlpSlot sl) {
#pragma clang fp contract(off)
    __shared__ OleAccLds<T> S;
    OlTileLds<T>& L = S.L;
    const OlLayerArgs proj = olp_choose(a.proj, sl);
    const int tid = threadIdx.x, M = a.M;
    const int d = tid & 15, s0 = tid >> 4, s1 = s0 + OL_THREADS / 16;
    double sum0 = a.acc[s0 * OLE_ACC_W + d], sum1 = a.acc[s1 * OLE_ACC_W + d];
    double cnt0 = 0.0, cnt1 = 0.0;
    if (d == 0) {
        cnt0 = a.acc[s0 * OLE_ACC_W + 16];
        cnt1 = a.acc[s1 * OLE_ACC_W + 16];
    }
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)proj.w, 512, 0, wf);
    for (int m0 = 0; m0 < M; m0 += 16) {
        ol_tile<T, false>(proj, L, 512, 0, m0, M, wf);
        if (tid < 16) {                               // as ol_tail_run: z, then z / sqrtf(ss), in f32
            float z[16], ss = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                z[k] = L.red[0][tid][k] + proj.bias[k];
                ss += z[k] * z[k];
            }
            const float nrm = sqrtf(ss);
#pragma unroll
            for (int k = 0; k < 16; ++k) S.zn[tid][k] = z[k] / nrm;
            int sl_ = -1;
            if (m0 + tid < M) {
                sl_ = a.slots[m0 + tid];
                if (sl_ < 0 || sl_ >= a.n_classes) sl_ = -1;
            }
            S.slot[tid] = sl_;
        }
        __syncthreads();
        for (int r = 0; r < 16; ++r) {                // the tile's windows in order
            const int c = S.slot[r];
            if (c == s0) {
                sum0 += (double)S.zn[r][d];
                cnt0 += 1.0;
            } else if (c == s1) {
                sum1 += (double)S.zn[r][d];
                cnt1 += 1.0;
            }
        }
        __syncthreads();                              // zn and slot are rewritten by the next tile
    }
    a.acc[s0 * OLE_ACC_W + d] = sum0;
    a.acc[s1 * OLE_ACC_W + d] = sum1;
    if (d == 0) {
        a.acc[s0 * OLE_ACC_W + 16] = cnt0;
        a.acc[s1 * OLE_ACC_W + 16] = cnt1;
    }
}
