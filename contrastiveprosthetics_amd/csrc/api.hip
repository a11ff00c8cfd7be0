// C ABI (include/cpnative.h) and the host-side sequencing of the contrastive step.
// One enqueue-only function per stage; no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>

#include "../../include/cpnative.h"
#include "common.cuh"
#include "gemm_nt.cuh"
#include "gemm_nt256p.cuh"
#include "gemm_ws.cuh"
#include "gemm_tn.cuh"
#include "gemm_tn256.cuh"
#include "kernels_misc.cuh"
#include "conv_kernels.cuh"
#include "head.cuh"
#include "optim.cuh"
#include "eval.cuh"
#include "preprocess.cuh"
#include "glove.cuh"
#include "fp8.cuh"
#include "small.cuh"
#include "online.cuh"
#include "online_adapt.cuh"
#include "online_multi.cuh"
#include "online_multi_adapt.cuh"
#include "online_enroll.cuh"
#include "online_finetune.cuh"
#include "online_gate.cuh"
#include "online_sequence.cuh"
#include "online_drive.cuh"
#include "online_subsets.cuh"
#include "online_maps.cuh"
#include "online_realign.cuh"
#include "online_track.cuh"
#include "online_holdout.cuh"
#include "online_prototypes.cuh"
#include "online_metric.cuh"
#include "online_readout.cuh"
#include "online_projections.cuh"
#include "online_kinematics.cuh"
#include "online_kalman.cuh"

static thread_local char g_err[512] = "";
static int fail(int code, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s (code %d%s%s)", what, code, code < 10000 ? ": " : "",
             code < 10000 ? hipGetErrorString((hipError_t)code) : "");
    return code;
}
#define CK(expr)                                         \
    do {                                                 \
        hipError_t e_ = (expr);                          \
        if (e_ != hipSuccess) return fail((int)e_, #expr); \
    } while (0)
#define CKL(what)                                        \
    do {                                                 \
        hipError_t e_ = hipGetLastError();               \
        if (e_ != hipSuccess) return fail((int)e_, what); \
    } while (0)

extern "C" int cp_version(void) { return CP_VERSION; }

// ---------------------------------------------------------------------------------------
// No process-wide switches: a call's options, tile schedule, synchronised-BatchNorm hook and gradient tap travel in its
// cp_config (include/cpnative.h).
// ---------------------------------------------------------------------------------------
static inline bool opt(const cp_config* c, uint32_t bit) { return (c->options & bit) != 0; }
extern "C" const char* cp_last_error(void) { return g_err; }

// tile schedule of the persistent fc GEMM kernels: cp_config.tile_schedule (cpnative.h)
static inline bool dyn_tiles(const cp_config* c) { return c->tile_schedule == CP_TILES_DYNAMIC; }

// ---------------------------------------------------------------------------------------
// optional per-kernel-kind timing with HIP events recorded on the launch stream
// (bench.py's live roofline measurement).  Events are created in cp_profile_enable, never
// inside a step.  Not thread-safe: one profiled stream at a time.
// ---------------------------------------------------------------------------------------
struct Profiler {
    bool on = false;
    uint64_t mask = 0;
    int cap = 0, used = 0;
    hipEvent_t* ev = nullptr;   // 2 per record
    int* kind = nullptr;
};
static Profiler g_prof;

struct ProfScope {
    hipStream_t st;
    int idx;
    ProfScope(int kind, hipStream_t s) : st(s), idx(-1) {
        if (g_prof.on && ((g_prof.mask >> kind) & 1) && g_prof.used < g_prof.cap) {
            idx = g_prof.used++;
            g_prof.kind[idx] = kind;
            (void)hipEventRecord(g_prof.ev[2 * idx], st);
        }
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(g_prof.ev[2 * idx + 1], st);
    }
};

extern "C" int cp_profile_enable(uint64_t kind_mask, int32_t max_records) {
    if (max_records <= 0) return fail(CP_ERR_ARG, "cp_profile_enable args");
    if (g_prof.cap < max_records) {
        for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
        delete[] g_prof.ev;
        delete[] g_prof.kind;
        g_prof.ev = new hipEvent_t[2 * (size_t)max_records];
        g_prof.kind = new int[max_records];
        for (int i = 0; i < 2 * max_records; ++i) CK(hipEventCreate(&g_prof.ev[i]));
        g_prof.cap = max_records;
    }
    g_prof.used = 0;
    g_prof.mask = kind_mask;
    g_prof.on = true;
    return 0;
}
extern "C" int cp_profile_disable(void) { g_prof.on = false; return 0; }
extern "C" int cp_profile_resume(void) {
    if (!g_prof.cap) return fail(CP_ERR_ARG, "cp_profile_resume before cp_profile_enable");
    g_prof.on = true;
    return 0;
}
extern "C" int cp_profile_summary(int32_t kind, double* total_ms, int64_t* count) {
    // caller has synchronised the stream
    if (!total_ms || !count) return fail(CP_ERR_ARG, "cp_profile_summary args");
    double t = 0;
    int64_t n = 0;
    for (int i = 0; i < g_prof.used; ++i)
        if (g_prof.kind[i] == kind) {
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
            t += ms;
            ++n;
        }
    *total_ms = t;
    *count = n;
    return 0;
}

// ---------------------------------------------------------------------------------------
// debug access: a stored tensor as f32 (cp_debug_activation, encoder_api.cuh)
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void to_f32_kernel(const T* __restrict__ in, float* __restrict__ out, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = DT<T>::load(in + i);
}

#include "encoder_api.cuh"            // the training encoder: workspace, cp_encoder_forward / cp_encoder_backward, cp_debug_activation / cp_debug_bn_stats

// ---------------------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------------------
extern "C" int cp_gather_groups(const float* table, int64_t table_rows, const int64_t* emg_rand, int64_t D,
                                const int64_t* perm, int64_t B, int32_t V, float* x_out, void* stream) {
    if (!table || !emg_rand || !perm || !x_out || B <= 0 || V <= 0) return fail(CP_ERR_ARG, "cp_gather_groups args");
    const int64_t total = B * CP_TASKS * V * 3;
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);      // (caps 1024 / 512 measured: 10.7 / 11.8 us against 10.7)
    ProfScope ps(CP_K_GATHER, (hipStream_t)stream);
    hipLaunchKernelGGL(gather_groups_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, emg_rand, perm, x_out,
                       B, CP_TASKS, (int)V, D, table_rows);
    CKL("gather_groups_kernel");
    return 0;
}

// sEMG augmentation in the gather's launch (an opt-in EXTENSION, no reference counterpart: include/cpnative.h, cp_augment).
// Everything is validated here, on the host, before the launch; nothing is allocated, synchronised or read.
extern "C" int cp_gather_groups_aug(const float* table, int64_t table_rows, const int64_t* emg_rand, int64_t D,
                                    const int64_t* perm, int64_t B, int32_t V, float* x_out, const cp_augment* aug, void* stream) {
    if (!table || !emg_rand || !perm || !x_out || B <= 0 || V <= 0) return fail(CP_ERR_ARG, "cp_gather_groups_aug args");
    if (!aug) return fail(CP_ERR_ARG, "cp_gather_groups_aug: aug is NULL");
    if ((((uintptr_t)table | (uintptr_t)x_out) & 15) != 0)                     // (rows are read and stored in 16-byte pieces)
        return fail(CP_ERR_ARG, "cp_gather_groups_aug: table and x_out must be 16-byte aligned");
    if (aug->shift_min < -7 || aug->shift_max > 7 || aug->shift_min > aug->shift_max)
        return fail(CP_ERR_ARG, "cp_gather_groups_aug: shift bounds must satisfy -7 <= shift_min <= shift_max <= 7");
    if (!(aug->p_drop >= 0.f && aug->p_drop <= 1.f)) return fail(CP_ERR_ARG, "cp_gather_groups_aug: p_drop outside [0, 1]");
    const float sig[3] = {aug->gain_sigma, aug->amp_sigma, aug->noise_sigma};
    for (int i = 0; i < 3; ++i)
        if (!(sig[i] >= 0.f && sig[i] <= 2.f))            // (a NaN fails both comparisons)
            return fail(CP_ERR_ARG, "cp_gather_groups_aug: gain_sigma, amp_sigma and noise_sigma must be finite and in [0, 2]");
    if (!std::isfinite(aug->fill)) return fail(CP_ERR_ARG, "cp_gather_groups_aug: fill must be finite");
    if (aug->dead_mask > 0xFFFu) return fail(CP_ERR_ARG, "cp_gather_groups_aug: dead_mask has bits above channel 11");
    const int64_t item_limit = (int64_t)1 << 32;
    if (aug->item_offset < 0 || aug->item_offset > item_limit || B > (item_limit - aug->item_offset) / CP_TASKS)
        return fail(CP_ERR_ARG, "cp_gather_groups_aug: item_offset + B * 41 must not exceed 2^32");
    GatherAugArgs a{};
    a.table = table; a.emg_rand = emg_rand; a.perm = perm; a.out = x_out; a.mean_std = aug->mean_std;
    a.salt_state = nullptr;
    if (aug->salt_state_lo || aug->salt_state_hi) {
        const uintptr_t st = ((uintptr_t)aug->salt_state_hi << 32) | aug->salt_state_lo;
        a.salt_state = &((const cp_step_state*)st)->aug_salt;
    }
    a.B = B; a.D = D; a.table_rows = table_rows; a.T = CP_TASKS; a.V = (int)V;
    a.seed = aug->seed; a.salt = aug->salt; a.item_offset = (uint32_t)aug->item_offset;
    a.drop_thresh = (uint32_t)floor((double)aug->p_drop * 65536.0 + 0.5);
    a.dead_mask = aug->dead_mask;
    a.shift_min = aug->shift_min; a.shift_span = aug->shift_max - aug->shift_min + 1;
    a.gain_sigma = aug->gain_sigma; a.amp_sigma = aug->amp_sigma; a.noise_sigma = aug->noise_sigma; a.fill = aug->fill;
    const int64_t total = B * CP_TASKS * V;               // one thread per window
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    ProfScope ps(CP_K_GATHER, (hipStream_t)stream);
    hipLaunchKernelGGL(gather_groups_aug_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    CKL("gather_groups_aug_kernel");
    return 0;
}

extern "C" int cp_gather_oob_count(uint32_t* count_out, int32_t reset, void* stream) {
    if (!count_out) return fail(CP_ERR_ARG, "cp_gather_oob_count args");
    unsigned int* ctr = nullptr;
    CK(hipGetSymbolAddress((void**)&ctr, HIP_SYMBOL(g_gather_oob)));
    CK(hipMemcpyAsync(count_out, ctr, sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (reset) CK(hipMemsetAsync(ctr, 0, sizeof(uint32_t), (hipStream_t)stream));
    return 0;
}


// ---------------------------------------------------------------------------------------
// head
// ---------------------------------------------------------------------------------------
extern "C" size_t cp_global_negatives_scratch_floats(int64_t n_all_windows) {
    return n_all_windows > 0 ? (size_t)n_all_windows + (size_t)2 * kHeadBlocksMax * GNEG_PART : 0;
}

// one workgroup per CU: each wave ends with 41 cross-lane sums, so several windows per thread beat more workgroups
// (tools/gneg_bench.py, 1 / 8 ranks' rows: 37 / 123 us with 256 workgroups, 59 / 153 with up to 1024)
extern "C" int cp_global_negatives_g(const cp_params* p, const float* z, int64_t n_windows, const int64_t* labels, float* scratch,
                                     float* gh, void* stream) {
    if (!p || !p->easy_w || !p->easy_b || !z || !labels || !scratch || !gh || n_windows <= 0 || n_windows % CP_TASKS != 0)
        return fail(CP_ERR_ARG, "cp_global_negatives_g args");
    hipStream_t st = (hipStream_t)stream;
    float* pos = scratch;
    float* part = scratch + n_windows;
    const int blocks = grid_rows(n_windows, 256, 256);
    ProfScope ps(CP_K_HEAD, st);
    hipLaunchKernelGGL(gneg_g_kernel, dim3(blocks), dim3(256), 0, st, z, n_windows, p->easy_w, p->easy_b, labels, part, pos);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(GNEG_PART)), dim3(FIN_THREADS), 0, st, part, blocks, GNEG_PART, gh);
    CKL("gneg_g kernels");
    return 0;
}

extern "C" int cp_global_negatives_h(int64_t n_windows, const int64_t* labels, float* scratch, float* gh, void* stream) {
    if (!labels || !scratch || !gh || n_windows <= 0 || n_windows % CP_TASKS != 0) return fail(CP_ERR_ARG, "cp_global_negatives_h args");
    hipStream_t st = (hipStream_t)stream;
    const float* pos = scratch;
    float* part2 = scratch + n_windows + (size_t)kHeadBlocksMax * GNEG_PART;
    const int blocks = grid_rows(n_windows, 256, 256);
    ProfScope ps(CP_K_HEAD, st);
    hipLaunchKernelGGL(gneg_h_kernel, dim3(blocks), dim3(256), 0, st, pos, n_windows, gh, labels, part2);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(GNEG_PART)), dim3(FIN_THREADS), 0, st, part2, blocks, GNEG_PART, gh + GNEG_PART);
    CKL("gneg_h kernels");
    return 0;
}

extern "C" int cp_global_negatives(const cp_params* p, const float* z_all, int64_t n_all_windows, const int64_t* labels,
                                   float* scratch, float* gh_out, void* stream) {
    if (int e = cp_global_negatives_g(p, z_all, n_all_windows, labels, scratch, gh_out, stream)) return e;
    return cp_global_negatives_h(n_all_windows, labels, scratch, gh_out, stream);
}

static int head_impl(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels, int64_t n_groups,
                     int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, float* loss_correct, int32_t* pred,
                     float* logits, cp_params* grads, const float* gneg, void* stream, bool temp = false,
                     const float* logit_scale = nullptr, float* d_logit_scale = nullptr);

extern "C" int cp_head(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels, int64_t n_groups,
                       int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, float* loss_correct, int32_t* pred,
                       float* logits, cp_params* grads, void* stream) {
    return head_impl(cfg, p, z, labels, n_groups, V, want_grad, ws, ws_bytes, loss_correct, pred, logits, grads, nullptr, stream);
}

extern "C" int cp_head_gneg(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels, int64_t n_groups,
                            int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, float* loss_correct, int32_t* pred,
                            float* logits, cp_params* grads, const float* gh, void* stream) {
    if (!gh || V != 1) return fail(CP_ERR_ARG, "cp_head_gneg: needs the {G, H} table of cp_global_negatives and V == 1 (training batches)");
    return head_impl(cfg, p, z, labels, n_groups, V, want_grad, ws, ws_bytes, loss_correct, pred, logits, grads, gh, stream);
}

// the temperature twin (include/cpnative.h): logits = exp(clamp(*logit_scale)) * cosines; the reference's per-group loss only
extern "C" int cp_head_temp(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels, int64_t n_groups,
                            int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, float* loss_correct, int32_t* pred,
                            float* logits, cp_params* grads, const float* logit_scale, float* d_logit_scale, void* stream) {
    if (!logit_scale) return fail(CP_ERR_ARG, "cp_head_temp: logit_scale (a device float) is NULL");
    if (want_grad && !d_logit_scale) return fail(CP_ERR_ARG, "cp_head_temp: gradients need d_logit_scale");
    return head_impl(cfg, p, z, labels, n_groups, V, want_grad, ws, ws_bytes, loss_correct, pred, logits, grads, nullptr, stream, true,
                     logit_scale, d_logit_scale);
}

static int head_impl(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels, int64_t n_groups,
                     int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, float* loss_correct, int32_t* pred,
                     float* logits, cp_params* grads, const float* gneg, void* stream, bool temp, const float* logit_scale,
                     float* d_logit_scale) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    // (n_groups % V: group g reads the z rows of batch entry g / V, V to a position -- a remainder would reach past n_windows)
    if (!p || !z || !labels || !loss_correct || !pred || V <= 0 || n_groups * CP_TASKS != cfg->n_windows || n_groups % V != 0)
        return fail(CP_ERR_ARG, gneg ? "cp_head_gneg args" : "cp_head args");
    if (want_grad && (!grads || !grads->easy_w || !grads->easy_b)) return fail(CP_ERR_ARG, gneg ? "cp_head_gneg grads" : "cp_head grads");
    if (((uintptr_t)z & 15) != 0)                                                                              // (head_kernel reads rows in 16-byte pieces)
        return fail(CP_ERR_ARG, gneg ? "cp_head_gneg: z must be 16-byte aligned" : "cp_head: z must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)ws;
    const size_t es = cfg->dtype == CP_F32 ? 4 : 2;
    ProfScope ps(CP_K_HEAD, st);
    // (no memset of dz: head_kernel writes whole 64-element rows, zeros in columns 16..63)
    HeadArgs a{};
    a.z = z; a.easy_w = p->easy_w; a.easy_b = p->easy_b; a.labels = labels;
    a.G = n_groups; a.V = V; a.want_grad = want_grad; a.dz_ld = 64; a.dz = base + w.dz;
    a.logits = logits; a.pred = pred; a.partials = (float*)(base + w.head_part);
    a.gneg = gneg;
    a.logit_scale = logit_scale;
    const int blocks = grid_rows(n_groups, HEAD_WAVES * (n_groups >= 2048 ? 2 : 1), kHeadBlocksMax);   // (>= 2048 groups: two per wave, half the prologues)
    // CP_FP8 (BASELINE config 4): the logits on the block-scaled 8-bit MFMA; "fp8_head_f32" keeps the f32 products (tests)
    const bool f8l = cfg->dtype == CP_FP8 && !opt(cfg, CP_OPT_FP8_HEAD_F32);
    if (temp) {
        if (cfg->dtype == CP_F32) hipLaunchKernelGGL((head_kernel<float, false, false, false, true>), dim3(blocks), dim3(256), 0, st, a);
        else if (f8l) hipLaunchKernelGGL((head_kernel<bf16_t, false, false, true, true>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((head_kernel<bf16_t, false, false, false, true>), dim3(blocks), dim3(256), 0, st, a);
    } else if (cfg->dtype != CP_F32) {
        if (f8l) {
            if (gneg) hipLaunchKernelGGL((head_kernel<bf16_t, false, true, true>), dim3(blocks), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((head_kernel<bf16_t, false, false, true>), dim3(blocks), dim3(256), 0, st, a);
        } else {
            if (gneg) hipLaunchKernelGGL((head_kernel<bf16_t, false, true>), dim3(blocks), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((head_kernel<bf16_t>), dim3(blocks), dim3(256), 0, st, a);
        }
    } else {
        if (gneg) hipLaunchKernelGGL((head_kernel<float, false, true>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((head_kernel<float>), dim3(blocks), dim3(256), 0, st, a);
    }
    CKL("head_kernel");
    int nr = blocks;
    const PreReduce pre{a.partials, (float*)(base + w.partials2), st};
    const float* pp = pre(nr, HEAD_PART, 2 * REDUCE_SLICES);
    hipLaunchKernelGGL(head_finalize_kernel, dim3(1), dim3(256), 0, st, pp, nr, n_groups, p->easy_w, p->easy_b,
                       want_grad, loss_correct, want_grad ? grads->easy_w : nullptr, want_grad ? grads->easy_b : nullptr,
                       logit_scale, (temp && want_grad) ? d_logit_scale : nullptr);
    CKL("head_finalize_kernel");
    return 0;
}

// debug access: the dL/dz rows the last cp_head / cp_head_gneg / cp_head_glove call with want_grad left in ws, all 64 columns, as f32
extern "C" int cp_debug_head_grad(const cp_config* cfg, void* ws, size_t ws_bytes, float* out, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (!out) return fail(CP_ERR_ARG, "cp_debug_head_grad args");
    const int64_t n = cfg->n_windows * HEAD_LD;
    unsigned char* base = (unsigned char*)ws;
    const hipStream_t st = (hipStream_t)stream;
    return by_dtype(cfg->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((to_f32_kernel<T>), dim3(1024), dim3(256), 0, st, (const T*)(base + w.dz), out, n);
        CKL("to_f32_kernel");
        return 0;
    });
}

extern "C" int cp_vote(const int32_t* pred, const int64_t* labels, int64_t B, int32_t V, float* curve, int32_t* y_pred,
                       void* stream) {
    if (!pred || !labels || !curve || !y_pred || B <= 0 || V <= 0 || V > 32) return fail(CP_ERR_ARG, "cp_vote args");
    hipLaunchKernelGGL(vote_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, pred, labels, B, (int)V, curve, y_pred);
    CKL("vote_kernel");
    return 0;
}

extern "C" int cp_subset_vote(const float* logits, const int64_t* labels, int64_t B, int32_t V, const uint8_t* masks,
                              int64_t n_masks, int64_t* correct, int32_t* y_pred, void* stream) {
    if (!logits || !labels || !masks || !correct || B <= 0 || B > 65535 || V <= 0 || V > SV_VMAX || n_masks <= 0)
        return fail(CP_ERR_ARG, "cp_subset_vote args");
    hipStream_t st = (hipStream_t)stream;
    CK(hipMemsetAsync(correct, 0, (size_t)n_masks * V * sizeof(int64_t), st));
    SubsetVoteArgs a{};
    a.logits = logits; a.labels = labels; a.masks = masks; a.correct = (unsigned long long*)correct; a.y_pred = y_pred;
    a.B = B; a.n_masks = n_masks; a.V = V;
    const size_t lds = sv_lds_bytes(V);
    static bool attr_set = false;
    if (!attr_set) {      // > 64 KiB of dynamic LDS needs the opt-in once per process
        CK(hipFuncSetAttribute((const void*)subset_vote_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sv_lds_bytes(SV_VMAX)));
        attr_set = true;
    }
    hipLaunchKernelGGL(subset_vote_kernel, dim3((unsigned)((n_masks + SV_MPB - 1) / SV_MPB), (unsigned)B), dim3(256), lds, st, a);
    CKL("subset_vote_kernel");
    return 0;
}

extern "C" int cp_confusion(const int32_t* y_pred, const int64_t* labels, int64_t n_groups, int64_t* counts, void* stream) {
    if (!y_pred || !labels || !counts || n_groups <= 0) return fail(CP_ERR_ARG, "cp_confusion args");
    const int64_t n = n_groups * SV_T;
    const int g = (int)((n + 255) / 256 > 256 ? 256 : (n + 255) / 256);
    hipLaunchKernelGGL(confusion_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, y_pred, labels, n, (unsigned long long*)counts);
    CKL("confusion_kernel");
    return 0;
}

extern "C" int cp_preprocess_emg(const float* raw, int64_t n_segments, int32_t seg_len, const double* b, const double* a,
                                 int32_t n_coef, int32_t rms_window, float gain, const int32_t* time_idx, int32_t n_out,
                                 float* out, void* stream) {
    if (!raw || !b || !a || !time_idx || !out || n_segments <= 0 || n_coef < 2 || n_coef > PP_MAXCOEF || a[0] == 0.0 ||
        rms_window < 1 || rms_window > PP_MAXWIN || n_out <= 0 || n_out > PP_MAXOUT || seg_len < rms_window ||
        seg_len > 2147483647 - 16)                         // the kernel indexes 16 samples ahead of t in int
        return fail(CP_ERR_ARG, "cp_preprocess_emg args");
    PreprocArgs p{};
    p.raw = raw; p.out = out; p.S = n_segments; p.L = seg_len; p.n_out = n_out; p.n_coef = n_coef; p.win = rms_window; p.gain = gain;
    for (int i = 0; i < n_coef; ++i) { p.b[i] = b[i] / a[0]; p.a[i] = a[i] / a[0]; }
    const int half = rms_window / 2, n_rms = seg_len - 2 * half;
    // keep list sorted by time (stable), so a thread walks it once while the series streams by
    int order[PP_MAXOUT];
    for (int i = 0; i < n_out; ++i) {
        if (time_idx[i] < 0 || time_idx[i] >= n_rms) return fail(CP_ERR_ARG, "cp_preprocess_emg: time_idx outside the RMS series");
        order[i] = i;
    }
    for (int i = 1; i < n_out; ++i) {
        const int v = order[i];
        int k = i - 1;
        while (k >= 0 && time_idx[order[k]] > time_idx[v]) { order[k + 1] = order[k]; --k; }
        order[k + 1] = v;
    }
    for (int i = 0; i < n_out; ++i) { p.t_sorted[i] = time_idx[order[i]]; p.slot_sorted[i] = (short)order[i]; }
    const int64_t threads = n_segments * PP_C;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (n_coef == 9 && rms_window == 11) hipLaunchKernelGGL((preprocess_kernel<9, 11>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((preprocess_kernel<0, 0>), grid, dim3(256), 0, (hipStream_t)stream, p);
    CKL("preprocess_kernel");
    return 0;
}

extern "C" int cp_emg_stats(const float* seg, int64_t n_segments, int32_t n_out, const uint8_t* use, int32_t complete,
                            double* scratch, float* mean_std, void* stream) {
    if (!seg || !scratch || !mean_std || n_segments < 2 || n_out <= 0) return fail(CP_ERR_ARG, "cp_emg_stats args");
    hipStream_t st = (hipStream_t)stream;
    const int64_t threads = n_segments * PP_C;
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, seg, n_segments, (int)n_out, scratch);
    hipLaunchKernelGGL(emg_stats_kernel, dim3(1), dim3(256), 0, st, scratch, use, n_segments, (int)complete, mean_std);
    CKL("emg_stats_kernel");
    return 0;
}

extern "C" int cp_emg_normalize(float* seg, int64_t n_rows, const float* mean_std, void* stream) {
    if (!seg || !mean_std || n_rows <= 0) return fail(CP_ERR_ARG, "cp_emg_normalize args");
    const int64_t n = n_rows * PP_C;
    const int g = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(emg_normalize_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, seg, n, mean_std);
    CKL("emg_normalize_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------
// glove-angle class encoder
// ---------------------------------------------------------------------------------------
struct GWS {
    size_t xp, w1p, h, a, w2p, w2t, dzg, gbuf, stats, coef, zeros, partials, partials2, slabs, frags, total;
};
static const int kGlovePartialRows = 2048, kGloveSlabs = 128;
static const int kGloveBwdBlocks = 512;       // workgroups (= f32 weight-gradient slabs of up to 32 KiB) of the fused glove backward kernels

// (CP_FP8 configurations run the glove-angle class encoder -- 0.3 % of the step's FLOPs, K = 20 -- on the bf16 kernels: 8-bit storage
//  is for the sEMG encoder's activations)
static GWS carve_glove(int64_t rows, int dtype) {
    const size_t es = dtype == CP_F32 ? 4 : 2;
    GWS g{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return o; };
    g.xp = take((size_t)rows * GL_KP * es);
    g.w1p = take((size_t)GL_H * GL_KP * es);
    g.h = take((size_t)rows * GL_H * es);
    g.a = take((size_t)rows * GL_H * es);
    g.w2p = take((size_t)32 * GL_H * es);
    g.w2t = take((size_t)GL_H * 64 * es);
    g.dzg = take((size_t)rows * 64 * es);
    g.gbuf = take((size_t)rows * GL_H * es);
    g.stats = take(4 * GL_H * 4);
    g.coef = take(3 * GL_H * 4);
    g.zeros = take(GL_H * 4);
    const int64_t tiles = (rows + 127) / 128;
    g.partials = take((size_t)(tiles > kGlovePartialRows ? tiles : kGlovePartialRows) * 2 * GL_H * 4);
    g.partials2 = take((size_t)REDUCE_SLICES * 2048 * 4);
    g.slabs = take((size_t)kGloveSlabs * 64 * GL_H * 4 > (size_t)kGloveBwdBlocks * GL_H * 32 * 4 ? (size_t)kGloveSlabs * 64 * GL_H * 4
                                                                                                  : (size_t)kGloveBwdBlocks * GL_H * 32 * 4);
    g.frags = take((size_t)GLF_COUNT * 64 * 16);
    g.total = off;
    return g;
}

extern "C" size_t cp_glove_workspace_bytes(int64_t max_rows, int32_t dtype) {
    if (max_rows <= 0 || (dtype != CP_F32 && dtype != CP_BF16 && dtype != CP_FP8)) return 0;
    return carve_glove(max_rows, dtype).total;
}

static int check_glove(const cp_config* c, int64_t rows, void* gws, size_t gws_bytes, GWS* out) {
    if (!c || !gws) return fail(CP_ERR_ARG, "null config/glove workspace");
    if (rows <= 0 || rows % CP_TASKS != 0) return fail(CP_ERR_ARG, "glove rows must be a positive multiple of 41");
    if (c->dtype != CP_F32 && c->dtype != CP_BF16 && c->dtype != CP_FP8) return fail(CP_ERR_ARG, "dtype");
    *out = carve_glove(rows, c->dtype);
    if (out->total > gws_bytes) return fail(CP_ERR_WORKSPACE, "glove workspace too small");
    if (((uintptr_t)gws & 255) != 0) return fail(CP_ERR_ARG, "glove workspace must be 256-byte aligned");
    return 0;
}

template <typename T>
static int glove_forward_t(const cp_config* c, const cp_glove_params* gp, const float* glove, int64_t R, unsigned char* base,
                           const GWS& w, float* zg, hipStream_t st) {
    const bool batch_stats = c->training || c->adabn;
    const bool have_running = gp->running_mean && gp->running_var;
    if (!batch_stats && !have_running) return fail(CP_ERR_ARG, "eval with stock BN needs running statistics");
    const int upd = (c->training && !c->adabn && have_running) ? 1 : 0;
    T* xp = (T*)(base + w.xp);
    T* h = (T*)(base + w.h);
    T* av = (T*)(base + w.a);
    float* partials = (float*)(base + w.partials);
    float* stats = (float*)(base + w.stats);
    if constexpr (sizeof(T) == 2) {
        // 16-bit storage, round 4 (glove.cuh): the hidden layer is recomputed from the 20 inputs, never stored -- statistics, then
        // relu(BN(.)) and the 256 -> 16 product in one kernel; no padded-K GEMM launches, no element-wise passes
        GloveFusedArgs fa{};
        fa.x = glove; fa.w1 = gp->w1; fa.w2 = gp->last_w; fa.stats = stats; fa.zg = zg; fa.partials = partials; fa.R = R;
        fa.xp = c->training ? (bf16_t*)xp : nullptr;                      // (the weight gradient's operand: training only)
        fa.frags = (const uint4*)(base + w.frags);
        hipLaunchKernelGGL(glove_prep_kernel, dim3(GLF_COUNT), dim3(64), 0, st, gp->w1, gp->last_w, (uint4*)(base + w.frags));
        const int64_t ntile = (R + 15) / 16;
        int nrows = (int)(ntile < kGlovePartialRows ? ntile : kGlovePartialRows);
        if (batch_stats) {
            hipLaunchKernelGGL(glove_stats_kernel, dim3(nrows), dim3(256), 0, st, fa);
            CKL("glove_stats_kernel");
        }
        hipLaunchKernelGGL(bn_finalize_kernel, dim3(FIN_GRID(GL_H)), dim3(FIN_THREADS), 0, st, partials, nrows, (double)R, gp->bn_g, gp->bn_b,
                           have_running ? gp->running_mean : nullptr, have_running ? gp->running_var : nullptr, upd,
                           batch_stats ? 0 : 1, c->bn_momentum, c->bn_eps, stats, GL_H);
        CKL("bn_finalize_kernel(glove)");
        const int gf = (int)((ntile + 3) / 4 < 2048 ? (ntile + 3) / 4 : 2048);
        hipLaunchKernelGGL(glove_fwd_kernel, dim3(gf), dim3(256), 0, st, fa);
        CKL("glove_fwd_kernel");
        return 0;
    }
    CK(hipMemsetAsync(base + w.zeros, 0, GL_H * 4, st));
    hipLaunchKernelGGL((pad_cast_kernel<T>), dim3(grid_rows(R * GL_KP, 256, 4096)), dim3(256), 0, st, glove, R, GL_IN, xp, R, GL_KP);
    hipLaunchKernelGGL((pad_cast_kernel<T>), dim3(64), dim3(256), 0, st, gp->w1, (int64_t)GL_H, GL_IN, (T*)(base + w.w1p), (int64_t)GL_H, GL_KP);
    hipLaunchKernelGGL((pad_cast_kernel<T>), dim3(32), dim3(256), 0, st, gp->last_w, (int64_t)CP_D_E, GL_H, (T*)(base + w.w2p), (int64_t)32, GL_H);
    CKL("pad_cast_kernel");
    {
        GemmNTArgs a{};
        a.A = xp; a.lda = GL_KP; a.M = R; a.K = GL_KP; a.W = base + w.w1p; a.F = GL_H;
        a.C = h; a.ldc = GL_H; a.bias = (float*)(base + w.zeros); a.relu = 0; a.partials = partials;
        CK((launch_gemm_nt<T, 128, 128, ALOAD_PLAIN, EPI_FWD>(a, st)));
    }
    {
        int nrows = (int)((R + 127) / 128);
        const PreReduce pre{partials, (float*)(base + w.partials2), st};
        const float* pp = batch_stats ? pre(nrows, 2 * GL_H) : partials;
        hipLaunchKernelGGL(bn_finalize_kernel, dim3(FIN_GRID(GL_H)), dim3(FIN_THREADS), 0, st, pp, nrows, (double)R, gp->bn_g, gp->bn_b,
                           have_running ? gp->running_mean : nullptr, have_running ? gp->running_var : nullptr, upd,
                           batch_stats ? 0 : 1, c->bn_momentum, c->bn_eps, stats, GL_H);
        CKL("bn_finalize_kernel(glove)");
    }
    hipLaunchKernelGGL((bn_relu_apply_kernel<T>), dim3(grid_rows(R * GL_H / DT<T>::EPC, 256, 4096)), dim3(256), 0, st, h, stats, av, R, GL_H);
    CKL("bn_relu_apply_kernel");
    {
        GemmNTArgs a{};
        a.A = av; a.lda = GL_H; a.M = R; a.K = GL_H; a.W = base + w.w2p; a.F = 32;
        a.C = zg; a.ldc = CP_D_E; a.f_valid = CP_D_E;
        CK((launch_gemm_nt<T, 128, 32, ALOAD_PLAIN, EPI_PLAIN_F32>(a, st)));
    }
    return 0;
}

extern "C" int cp_glove_forward(const cp_config* cfg, const cp_glove_params* gp, const float* glove, int64_t rows,
                                void* gws, size_t gws_bytes, float* zg, void* stream) {
    GWS w;
    if (int e = check_glove(cfg, rows, gws, gws_bytes, &w)) return e;
    if (!gp || !gp->w1 || !gp->bn_g || !gp->bn_b || !gp->last_w || !glove || !zg) return fail(CP_ERR_ARG, "cp_glove_forward args");
    // (the fused kernels read glove rows and store zg rows in 16-byte pieces; rows are 80 and 64 bytes)
    if (((uintptr_t)glove & 15) != 0) return fail(CP_ERR_ARG, "cp_glove_forward: glove must be 16-byte aligned");
    if (((uintptr_t)zg & 15) != 0) return fail(CP_ERR_ARG, "cp_glove_forward: zg must be 16-byte aligned");
    if (cfg->dtype != CP_F32) return glove_forward_t<bf16_t>(cfg, gp, glove, rows, (unsigned char*)gws, w, zg, (hipStream_t)stream);
    return glove_forward_t<float>(cfg, gp, glove, rows, (unsigned char*)gws, w, zg, (hipStream_t)stream);
}

static int head_glove_impl(const cp_config* cfg, const float* z, const float* zg, const int64_t* labels, int64_t n_groups,
                           int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, void* gws, size_t gws_bytes,
                           float* loss_correct, int32_t* pred, float* logits, void* stream, bool temp, const float* logit_scale,
                           float* d_logit_scale);

extern "C" int cp_head_glove(const cp_config* cfg, const float* z, const float* zg, const int64_t* labels, int64_t n_groups,
                             int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, void* gws, size_t gws_bytes,
                             float* loss_correct, int32_t* pred, float* logits, void* stream) {
    return head_glove_impl(cfg, z, zg, labels, n_groups, V, want_grad, ws, ws_bytes, gws, gws_bytes, loss_correct, pred, logits, stream,
                           false, nullptr, nullptr);
}

extern "C" int cp_head_glove_temp(const cp_config* cfg, const float* z, const float* zg, const int64_t* labels, int64_t n_groups,
                                  int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, void* gws, size_t gws_bytes,
                                  float* loss_correct, int32_t* pred, float* logits, const float* logit_scale, float* d_logit_scale,
                                  void* stream) {
    if (!logit_scale) return fail(CP_ERR_ARG, "cp_head_glove_temp: logit_scale (a device float) is NULL");
    if (want_grad && !d_logit_scale) return fail(CP_ERR_ARG, "cp_head_glove_temp: gradients need d_logit_scale");
    return head_glove_impl(cfg, z, zg, labels, n_groups, V, want_grad, ws, ws_bytes, gws, gws_bytes, loss_correct, pred, logits, stream,
                           true, logit_scale, d_logit_scale);
}

static int head_glove_impl(const cp_config* cfg, const float* z, const float* zg, const int64_t* labels, int64_t n_groups,
                           int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, void* gws, size_t gws_bytes,
                           float* loss_correct, int32_t* pred, float* logits, void* stream, bool temp, const float* logit_scale,
                           float* d_logit_scale) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (!z || !zg || !labels || !loss_correct || !pred || V <= 0 || n_groups * CP_TASKS != cfg->n_windows || n_groups % V != 0)
        return fail(CP_ERR_ARG, "cp_head_glove args");
    if (want_grad && V != 1) return fail(CP_ERR_ARG, "cp_head_glove: gradients need V == 1 (training batches)");
    if (((uintptr_t)z & 15) != 0) return fail(CP_ERR_ARG, "cp_head_glove: z must be 16-byte aligned");        // (head_kernel reads rows in 16-byte pieces)
    if (((uintptr_t)zg & 15) != 0) return fail(CP_ERR_ARG, "cp_head_glove: zg must be 16-byte aligned");
    const int64_t R = n_groups / V * CP_TASKS;
    GWS gw;
    if (int e = check_glove(cfg, R, gws, gws_bytes, &gw)) return e;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)ws;
    unsigned char* gbase = (unsigned char*)gws;
    ProfScope ps(CP_K_HEAD, st);
    // (no memsets of dz / dzg: head_kernel writes whole 64-element rows)
    HeadArgs a{};
    a.z = z; a.labels = labels; a.zg = zg; a.dzg = gbase + gw.dzg; a.dzg_ld = 64;
    a.G = n_groups; a.V = V; a.want_grad = want_grad; a.dz_ld = 64; a.dz = base + w.dz;
    a.logits = logits; a.pred = pred; a.partials = (float*)(base + w.head_part);
    a.logit_scale = logit_scale;
    const int blocks = grid_rows(n_groups, HEAD_WAVES * (n_groups >= 2048 ? 2 : 1), kHeadBlocksMax);   // (>= 2048 groups: two per wave, half the prologues)
    if (temp && cfg->dtype != CP_F32)
        hipLaunchKernelGGL((head_kernel<bf16_t, true, false, false, true>), dim3(blocks), dim3(256), 0, st, a);
    else if (temp)
        hipLaunchKernelGGL((head_kernel<float, true, false, false, true>), dim3(blocks), dim3(256), 0, st, a);
    else if (cfg->dtype != CP_F32)
        hipLaunchKernelGGL((head_kernel<bf16_t, true>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((head_kernel<float, true>), dim3(blocks), dim3(256), 0, st, a);
    CKL("head_kernel<glove>");
    int nr = blocks;
    const PreReduce pre{a.partials, (float*)(base + w.partials2), st};
    const float* pp = pre(nr, HEAD_PART, 2 * REDUCE_SLICES);
    hipLaunchKernelGGL(head_finalize_kernel, dim3(1), dim3(256), 0, st, pp, nr, n_groups, (const float*)nullptr, (const float*)nullptr,
                       0, loss_correct, (float*)nullptr, (float*)nullptr, logit_scale, (temp && want_grad) ? d_logit_scale : nullptr);
    CKL("head_finalize_kernel");
    return 0;
}

// debug access: the dL/dzg rows the last cp_head_glove call with want_grad left in gws, all 64 columns, as f32
extern "C" int cp_debug_glove_head_grad(const cp_config* cfg, void* gws, size_t gws_bytes, int64_t rows, float* out, void* stream) {
    GWS w;
    if (int e = check_glove(cfg, rows, gws, gws_bytes, &w)) return e;
    if (!out) return fail(CP_ERR_ARG, "cp_debug_glove_head_grad args");
    const int64_t n = rows * HEAD_LD;
    unsigned char* base = (unsigned char*)gws;
    const hipStream_t st = (hipStream_t)stream;
    return by_dtype(cfg->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((to_f32_kernel<T>), dim3(1024), dim3(256), 0, st, (const T*)(base + w.dzg), out, n);
        CKL("to_f32_kernel");
        return 0;
    });
}

template <typename T>
static int glove_backward_t(const cp_config* c, const cp_glove_params* gp, int64_t R, unsigned char* base, const GWS& w,
                            cp_glove_params* g, hipStream_t st) {
    using D = DT<T>;
    T* xp = (T*)(base + w.xp);
    T* h = (T*)(base + w.h);
    T* av = (T*)(base + w.a);
    T* dzg = (T*)(base + w.dzg);
    T* gbuf = (T*)(base + w.gbuf);
    float* partials = (float*)(base + w.partials);
    float* slabs = (float*)(base + w.slabs);
    float* stats = (float*)(base + w.stats);
    float* coef = (float*)(base + w.coef);
    const PreReduce pre{partials, (float*)(base + w.partials2), st};
    int S;
    if constexpr (sizeof(T) == 2) {
        // 16-bit storage, round 4 (glove.cuh): two recompute kernels around the coefficient launch -- the first reduces the
        // BatchNorm-backward sums and forms dW2 = dzg^T relu(BN(h)), the second forms dW1 = (dL/dh)^T x; both weight gradients run on the
        // matrix pipe inside them (per-workgroup f32 slabs, summed in fixed order) and no row-sized tensor is written
        GloveFusedArgs fa{};
        fa.xp = (bf16_t*)xp; fa.w1 = gp->w1; fa.w2 = gp->last_w; fa.stats = stats; fa.coef = coef; fa.dzg = (const bf16_t*)dzg;
        fa.slabs = slabs; fa.partials = partials; fa.R = R;
        fa.frags = (const uint4*)(base + w.frags);                          // (made by the forward pass: the weights have not moved since)
        const int64_t npair = (R + 31) / 32;
        const int nb = (int)(npair < kGloveBwdBlocks ? npair : kGloveBwdBlocks);
        hipLaunchKernelGGL(glove_bwd_kernel<0>, dim3(nb), dim3(256), 0, st, fa);
        hipLaunchKernelGGL(glove_reduce_kernel, dim3(CP_D_E * GL_H / 64), dim3(256), 0, st, slabs, nb, CP_D_E, GL_H, GL_H, g->last_w);
        CKL("glove_bwd_kernel<0>");
        int nr = nb;
        const float* pp = pre(nr, 2 * GL_H);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(FIN_GRID(GL_H)), dim3(FIN_THREADS), 0, st, pp, nr, (double)R, stats, coef, g->bn_g, g->bn_b, GL_H, 1);
        CKL("bn_bwd_finalize_kernel(glove)");
        hipLaunchKernelGGL(glove_bwd_kernel<1>, dim3(nb), dim3(256), 0, st, fa);
        hipLaunchKernelGGL(glove_reduce_kernel, dim3((GL_H * GL_IN + 63) / 64), dim3(256), 0, st, slabs, nb, GL_H, 32, GL_IN, g->w1);
        CKL("glove_bwd_kernel<1>");
        (void)S; (void)av; (void)gbuf;
        return 0;
    }
    // last: dW2 = dzg^T a   and   da = dzg W2
    hipLaunchKernelGGL((transpose_w_kernel<T>), dim3(64), dim3(256), 0, st, gp->last_w, (T*)(base + w.w2t), CP_D_E, GL_H, 64, 0);
    CKL("transpose_w_kernel(glove)");
    {
        GemmTNArgs ta{};
        ta.X = dzg; ta.ldx = 64; ta.Y = av; ta.ldy = GL_H; ta.slabs = slabs; ta.M = R; ta.P = 64; ta.Q = GL_H;
        split_rows(R, kGloveSlabs, &S, &ta.rows_per_split);
        CK((launch_gemm_tn<T, 64, 128, YLOAD_PLAIN>(ta, S, st)));
        hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(32), dim3(256), 0, st, slabs, S, 64, GL_H, CP_D_E, (const float*)nullptr,
                           (const float*)nullptr, (const float*)nullptr, g->last_w, 0, (float*)nullptr);
        CKL("reduce_slabs(glove last)");
    }
    {
        GemmNTArgs a{};
        a.A = dzg; a.lda = 64; a.M = R; a.K = 64; a.W = base + w.w2t; a.F = GL_H;
        a.C = gbuf; a.ldc = GL_H; a.R = nullptr; a.ldr = GL_H; a.partials = partials;
        CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, nullptr, dyn_tiles(c))));
    }
    // ReLU backward + the BN-backward sums, the coefficients, BN backward
    {
        const int gb = grid_rows(R, 256 / (GL_H / D::EPC), kGlovePartialRows);
        const int rpp = 256 / (GL_H / D::EPC);
        hipLaunchKernelGGL((relu_bwd_colsum_kernel<T>), dim3(gb), dim3(256), (size_t)rpp * 2 * GL_H * 4, st, gbuf, av, h, partials, R, GL_H);
        CKL("relu_bwd_colsum_kernel");
        int nr = gb;
        const float* pp = pre(nr, 2 * GL_H);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(FIN_GRID(GL_H)), dim3(FIN_THREADS), 0, st, pp, nr, (double)R, stats, coef, g->bn_g, g->bn_b, GL_H, 1);
        CKL("bn_bwd_finalize_kernel(glove)");
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(grid_rows(R * GL_H / D::EPC, 256, 4096)), dim3(256), 0, st, gbuf, h, coef, R, GL_H);
        CKL("bn_bwd_apply_kernel");
    }
    // first Linear: dW1^T = xp^T dh, reduced into the (256,20) layout
    {
        GemmTNArgs ta{};
        ta.X = xp; ta.ldx = GL_KP; ta.Y = gbuf; ta.ldy = GL_H; ta.slabs = slabs; ta.M = R; ta.P = 64; ta.Q = GL_H;
        split_rows(R, kGloveSlabs, &S, &ta.rows_per_split);
        CK((launch_gemm_tn<T, 64, 128, YLOAD_PLAIN>(ta, S, st)));
        hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(32), dim3(256), 0, st, slabs, S, 64, GL_H, GL_IN, (const float*)nullptr,
                           (const float*)nullptr, (const float*)nullptr, g->w1, 3, (float*)nullptr);
        CKL("reduce_slabs(glove w1)");
    }
    return 0;
}

extern "C" int cp_glove_backward(const cp_config* cfg, const cp_glove_params* gp, int64_t rows, void* gws, size_t gws_bytes,
                                 cp_glove_params* grads, void* stream) {
    GWS w;
    if (int e = check_glove(cfg, rows, gws, gws_bytes, &w)) return e;
    if (!gp || !gp->last_w || !grads || !grads->w1 || !grads->bn_g || !grads->bn_b || !grads->last_w)
        return fail(CP_ERR_ARG, "cp_glove_backward args");
    if (cfg->dtype != CP_F32) return glove_backward_t<bf16_t>(cfg, gp, rows, (unsigned char*)gws, w, grads, (hipStream_t)stream);
    return glove_backward_t<float>(cfg, gp, rows, (unsigned char*)gws, w, grads, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// optimiser
// ---------------------------------------------------------------------------------------
// the table as the kernels take it.  Refused here, before any launch: a negative numel (a negative chunk count, and a grid that no
// longer matches the table) and a negative offset (an index in front of the buffers)
static int build_opt(const char* who, OptArgs* a, const int64_t* off, const int64_t* numel, const int32_t* group, const int32_t* l2, int n) {
    char msg[160];
    if (n <= 0 || n > CP_MAX_TENSORS || !off || !numel || !group || !l2) {
        snprintf(msg, sizeof(msg), "%s: tensor table (n = %d, 1..%d entries)", who, n, CP_MAX_TENSORS);
        return fail(CP_ERR_ARG, msg);
    }
    int64_t chunk = 0;
    for (int i = 0; i < n; ++i) {
        if (off[i] < 0 || numel[i] < 0) {
            snprintf(msg, sizeof(msg), "%s: tensor table entry %d has a negative %s (%lld)", who, i, off[i] < 0 ? "offset" : "numel",
                     (long long)(off[i] < 0 ? off[i] : numel[i]));
            return fail(CP_ERR_ARG, msg);
        }
        const int64_t nchunks = numel[i] / OPT_CHUNK + (numel[i] % OPT_CHUNK != 0);
        if (chunk + nchunks > INT32_MAX) {
            snprintf(msg, sizeof(msg), "%s: tensor table entry %d takes the table past 2^31 chunks", who, i);
            return fail(CP_ERR_ARG, msg);
        }
        a->t[i].offset = off[i];
        a->t[i].numel = numel[i];
        a->t[i].chunk0 = (int)chunk;
        a->t[i].nchunks = (int)nchunks;
        a->t[i].group = group[i] ? 1 : 0;
        a->t[i].l2 = l2[i] ? 1 : 0;
        chunk += nchunks;
    }
    if (chunk == 0) {                                    // (an empty grid is no launch)
        snprintf(msg, sizeof(msg), "%s: tensor table without an element", who);
        return fail(CP_ERR_ARG, msg);
    }
    a->n_tensors = n;
    a->total_chunks = (int)chunk;
    return 0;
}

extern "C" size_t cp_optimizer_scratch_floats(const int64_t* numel_host, int32_t n) {
    size_t chunks = 0;
    for (int i = 0; i < n; ++i) chunks += (size_t)((numel_host[i] + OPT_CHUNK - 1) / OPT_CHUNK);
    return chunks + CP_MAX_TENSORS + 64;
}

static int launch_norms(OptArgs& a, float* scratch, float* l2_out, hipStream_t st) {
    a.norm_partials = scratch;
    a.norms = scratch + a.total_chunks;
    a.l2_out = l2_out;
    hipLaunchKernelGGL(l2_sumsq_kernel, dim3(a.total_chunks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(l2_finalize_kernel, dim3(1), dim3(L2_FIN_LANES * CP_MAX_TENSORS), 0, st, a);
    CKL("l2 norms");
    return 0;
}

extern "C" int cp_l2_norms(const float* params_flat, const int64_t* offset_host, const int64_t* numel_host,
                           const int32_t* group_host, const int32_t* l2_host, int32_t n, const cp_adam_hyper* h,
                           float* scratch, float* l2_out, void* stream) {
    if (!params_flat || !h || !scratch || !l2_out) return fail(CP_ERR_ARG, "cp_l2_norms args");
    OptArgs a{};
    if (int e = build_opt("cp_l2_norms", &a, offset_host, numel_host, group_host, l2_host, n)) return e;
    a.p = const_cast<float*>(params_flat);
    a.reg[0] = h->reg_emg; a.reg[1] = h->reg_glove;
    return launch_norms(a, scratch, l2_out, (hipStream_t)stream);
}

extern "C" int cp_l2_adam_step(float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq,
                               const int64_t* offset_host, const int64_t* numel_host, const int32_t* group_host,
                               const int32_t* l2_host, int32_t n, const cp_adam_hyper* h, int64_t step_index, float* scratch,
                               float* l2_out, void* stream) {
    if (!params_flat || !grads_flat || !exp_avg || !exp_avg_sq || !h || !scratch || !l2_out || step_index < 1)
        return fail(CP_ERR_ARG, "cp_l2_adam_step args");
    OptArgs a{};
    if (int e = build_opt("cp_l2_adam_step", &a, offset_host, numel_host, group_host, l2_host, n)) return e;
    a.p = params_flat; a.g = grads_flat; a.m = exp_avg; a.v = exp_avg_sq;
    a.lr[0] = h->lr_emg; a.lr[1] = h->lr_glove; a.reg[0] = h->reg_emg; a.reg[1] = h->reg_glove;
    a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.grad_scale = h->grad_scale;
    a.bc1 = (float)(1.0 - pow((double)h->beta1, (double)step_index));
    a.bc2 = (float)(1.0 - pow((double)h->beta2, (double)step_index));
    ProfScope ps(CP_K_OPT, (hipStream_t)stream);
    a.norm_partials = scratch; a.norms = scratch + a.total_chunks; a.l2_out = l2_out;
    hipLaunchKernelGGL(l2_sumsq_kernel, dim3(a.total_chunks), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(adam_kernel<true>, dim3(a.total_chunks), dim3(256), 0, (hipStream_t)stream, a);      // (norms folded inside: optim.cuh)
    CKL("l2 norms + adam_kernel");
    return 0;
}

extern "C" int cp_l2_adam_step_graph(float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq,
                                     const int64_t* offset_host, const int64_t* numel_host, const int32_t* group_host,
                                     const int32_t* l2_host, int32_t n, const cp_adam_hyper* h, const cp_step_state* state_dev,
                                     float* scratch, float* l2_out, void* stream) {
    if (!params_flat || !grads_flat || !exp_avg || !exp_avg_sq || !h || !scratch || !l2_out || !state_dev)
        return fail(CP_ERR_ARG, "cp_l2_adam_step_graph args");
    OptArgs a{};
    if (int e = build_opt("cp_l2_adam_step_graph", &a, offset_host, numel_host, group_host, l2_host, n)) return e;
    a.p = params_flat; a.g = grads_flat; a.m = exp_avg; a.v = exp_avg_sq;
    a.lr[0] = h->lr_emg; a.lr[1] = h->lr_glove; a.reg[0] = h->reg_emg; a.reg[1] = h->reg_glove;
    a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.grad_scale = h->grad_scale;
    a.bc1 = a.bc2 = 1.f;
    a.state = (const float*)state_dev;
    ProfScope ps(CP_K_OPT, (hipStream_t)stream);
    a.norm_partials = scratch; a.norms = scratch + a.total_chunks; a.l2_out = l2_out;
    hipLaunchKernelGGL(l2_sumsq_kernel, dim3(a.total_chunks), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(adam_kernel<true>, dim3(a.total_chunks), dim3(256), 0, (hipStream_t)stream, a);      // (norms folded inside: optim.cuh)
    CKL("l2 norms + adam_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// debug access
// ---------------------------------------------------------------------------------------
template <typename T>
static int debug_fc_gemm_t(const cp_debug_fc_gemm_args* d, hipStream_t st) {
    const int64_t M = d->M;
    const int K = d->K, F = d->F;
    int rows = 0;
    if (d->kind == 2) {
        int S;
        if constexpr (sizeof(T) == 2) {
            GemmTN256Args ta{};
            ta.X = (const bf16_t*)d->A; ta.ldx = K; ta.Y = (const bf16_t*)d->W; ta.ldy = F; ta.slabs = (float*)d->C; ta.M = M; ta.P = K; ta.Q = F;
            split_rows(M, F == 512 ? 64 : 40, &S, &ta.rows_per_split);
            ta.splits = S;
            CK(launch_gemm_tn256(ta, st));
        } else {
            GemmTNArgs ta{};
            ta.X = d->A; ta.ldx = K; ta.Y = d->W; ta.ldy = F; ta.slabs = (float*)d->C; ta.M = M; ta.P = K; ta.Q = F;
            split_rows(M, 32, &S, &ta.rows_per_split);
            CK((launch_gemm_tn<T, 128, 128, YLOAD_PLAIN>(ta, S, st)));
        }
        if (d->stat_rows_out) *d->stat_rows_out = S;
        return 0;
    }
    GemmNTArgs a{};
    a.A = d->A; a.lda = K; a.M = M; a.K = K; a.W = d->W; a.F = F; a.C = d->C; a.ldc = F; a.bias = d->bias; a.relu = 1;
    a.R = d->R; a.ldr = F; a.partials = d->partials;
    a.coef = d->coef; a.coef_mod = d->coef ? d->coef_mod : 0;
    a.dp_thresh = d->dp_thresh; a.dp_key = d->dp_key; a.dp_inv_keep = d->dp_inv_keep;
    const bool dyn = d->tile_schedule == CP_TILES_DYNAMIC;
    if (d->kind == 0) CK((launch_fc_gemm<T, EPI_FWD>(a, st, &rows, dyn)));
    else CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, &rows, dyn)));
    if (d->kind == 1 && !d->R) rows = 0;                  // a data gradient without a saved activation carries no sums
    if (d->stat_rows_out) *d->stat_rows_out = rows;
    return 0;
}

// everything a launcher would refuse, or a kernel would read or write out of bounds, before anything launches
static int check_debug_fc_gemm(const cp_debug_fc_gemm_args* d) {
    if (!d) return fail(CP_ERR_ARG, "cp_debug_fc_gemm args");
    if (d->dtype != CP_F32 && d->dtype != CP_BF16) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: dtype must be CP_F32 or CP_BF16");
    if (d->kind < 0 || d->kind > 2) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: kind must be 0, 1 or 2");
    if (d->tile_schedule != CP_TILES_STATIC && d->tile_schedule != CP_TILES_DYNAMIC) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: tile_schedule");
    if (!d->A || !d->W || !d->C) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: A, W and C must not be NULL");
    if (d->kind != 2 && !d->partials) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: partials must not be NULL");
    if (d->kind == 0 && !d->bias) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: the forward needs a bias");
    if (d->M <= 0 || d->K <= 0 || d->F <= 0 || d->K % 64 || d->F % 256) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: M > 0, K % 64 == 0, F % 256 == 0");
    const bool b16 = d->dtype == CP_BF16;
    if (d->kind == 2 && d->K % (b16 ? 256 : 128)) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: the weight gradient needs K % 256 == 0 (f32: 128)");
    if (b16 && d->kind != 2 && d->F > 256 * NT256P_MAX_TILES_F) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: F > 768");
    // 32-bit byte offsets of the weight-stationary kernels' buffer loads and the dropout hash's 32-bit element index (check_cfg)
    const int wide = d->K > d->F ? d->K : d->F;
    if ((uint64_t)d->M * (uint64_t)wide * 2 >= 0xFFF00000ull) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: M * max(K, F) * 2 must stay below 2^32");
    const bool drop = d->dp_thresh != 0;
    if (d->kind != 1 && (d->R || d->coef || drop)) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: R, coef and dropout belong to kind 1");
    if ((d->coef || drop) && (!d->R || !b16)) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: coef and dropout need R and CP_BF16");
    if (d->coef && drop) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: coef and dropout exclude each other");
    if (d->coef && d->coef_mod <= 0) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: coef_mod must be positive");
    if (drop && (d->dp_thresh > 65535u || !(d->dp_inv_keep > 0.f))) return fail(CP_ERR_ARG, "cp_debug_fc_gemm: dp_thresh in 1..65535, dp_inv_keep > 0");
    if ((((uintptr_t)d->A | (uintptr_t)d->W | (uintptr_t)d->C | (uintptr_t)d->R) & 15) != 0)
        return fail(CP_ERR_ARG, "cp_debug_fc_gemm: A, W, C and R must be 16-byte aligned");
    return 0;
}

extern "C" int cp_debug_fc_gemm(const cp_debug_fc_gemm_args* args, void* stream) {
    if (int e = check_debug_fc_gemm(args)) return e;
    if (args->dtype == CP_BF16) return debug_fc_gemm_t<bf16_t>(args, (hipStream_t)stream);
    return debug_fc_gemm_t<float>(args, (hipStream_t)stream);
}

// One launch sequence of the large-batch conv front end on caller buffers, through the launch functions of the step
// (csrc/encoder_api.cuh: their grid arithmetic, slab counts and pre-reduce rule), at any n_windows
template <typename T>
static int debug_conv_t(const cp_debug_conv_args* d, hipStream_t st) {
    const ConvLaunch cl{st, d->n_windows, d->partials, d->slabs, d->fold, d->stats1};
    cp_params p{}, g{};
    p.conv1_w = const_cast<float*>(d->conv1_w); p.conv1_b = const_cast<float*>(d->conv1_b);
    p.conv2_w = const_cast<float*>(d->conv2_w); p.conv2_b = const_cast<float*>(d->conv2_b);
    T* wc_f = (T*)d->wc;
    T* wc_d = wc_f + 64 * 192;
    const bool g8 = d->gin_exp != nullptr;
    ConvArgs ca{};
    ca.x = d->x; ca.w1 = d->conv1_w; ca.b1 = d->conv1_b; ca.n_windows = d->n_windows;
    int rows = 0, gcol_rows = 0;
    if (d->kind != 0 && d->kind != 3) {
        launch_prep_conv2<T>(d->conv2_w, wc_f, wc_d, st);
        CKL("prep_conv2_kernel");
    }
    switch (d->kind) {
    case 0:
        if (int e = launch_conv1_stats<T>(cl, &p, d->x, nullptr, "conv1_stats_kernel", &rows)) return e;
        break;
    case 1:
        ca.stats1 = d->stats1; ca.wc = wc_f; ca.bias2 = d->conv2_b; ca.out = d->out; ca.partials = d->partials;
        if (int e = launch_conv2_fwd<T>(cl, ca, "conv2_strip_kernel<fwd>", &rows)) return e;
        break;
    case 2:
        ca.wc = wc_d; ca.gin = d->gin; ca.out = d->out; ca.partials = d->partials;
        if (int e = launch_conv2_dgrad<T>(cl, ca, &rows)) return e;
        break;
    case 3: {
        // (as conv_backward_tail: the image holds the raw r1, stats1 is the finish kernel's)
        const float* gcols = d->gcols;
        gcol_rows = d->gcol_rows;
        if (!gcols) {
            if (int e = launch_conv2_gcols<T>(cl, (const T*)d->gin, &gcol_rows)) return e;
            gcols = d->partials;
        }
        ca.gin = d->gin; ca.gin_exp = (const int*)d->gin_exp;
        g.conv2_w = d->dw;
        if (int e = conv2_wgrad<T>(cl, &p, &g, ca, false, g8, gcols, gcol_rows, nullptr, nullptr, &rows)) return e;
        break;
    }
    default:
        ca.wc = wc_d; ca.gin = d->gin; ca.gin_exp = (const int*)d->gin_exp; ca.coef = d->coef; ca.partials = d->partials;
        if (int e = launch_conv2_dgrad_conv1<T>(cl, ca, false, g8, &rows)) return e;
        g.conv1_w = d->dw; g.conv1_b = d->db;
        if (int e = conv1_bwd_finalize(cl, rows, &g)) return e;
        break;
    }
    if (d->rows_out) *d->rows_out = rows;
    if (d->gcol_rows_out) *d->gcol_rows_out = gcol_rows;
    return 0;
}

// everything a launcher would refuse, or a kernel would read or write out of bounds, before anything launches
static int check_debug_conv(const cp_debug_conv_args* d) {
    if (!d) return fail(CP_ERR_ARG, "cp_debug_conv args");
    if (d->dtype != CP_F32 && d->dtype != CP_BF16) return fail(CP_ERR_ARG, "cp_debug_conv: dtype must be CP_F32 or CP_BF16");
    if (d->kind < 0 || d->kind > 4) return fail(CP_ERR_ARG, "cp_debug_conv: kind must be 0..4");
    if (d->n_windows <= 0) return fail(CP_ERR_ARG, "cp_debug_conv: n_windows must be positive");
    const int k = d->kind;
    if (!d->x || !d->conv1_w || !d->conv1_b) return fail(CP_ERR_ARG, "cp_debug_conv: x, conv1_w and conv1_b must not be NULL");
    if (k != 0 && !d->conv2_w) return fail(CP_ERR_ARG, "cp_debug_conv: conv2_w must not be NULL");
    if (k == 1 && !d->conv2_b) return fail(CP_ERR_ARG, "cp_debug_conv: the forward needs conv2_b");
    if ((k == 1 || k == 3) && !d->stats1) return fail(CP_ERR_ARG, "cp_debug_conv: kinds 1 and 3 need stats1");
    if (k >= 2 && !d->gin) return fail(CP_ERR_ARG, "cp_debug_conv: gin must not be NULL");
    if (k == 4 && !d->coef) return fail(CP_ERR_ARG, "cp_debug_conv: kind 4 needs coef");
    if (k != 0 && k != 3 && !d->wc) return fail(CP_ERR_ARG, "cp_debug_conv: wc must not be NULL");
    if ((k == 1 || k == 2) && !d->out) return fail(CP_ERR_ARG, "cp_debug_conv: out must not be NULL");
    if ((k != 3 || !d->gcols) && !d->partials) return fail(CP_ERR_ARG, "cp_debug_conv: partials must not be NULL");
    if (k == 3 && !d->slabs) return fail(CP_ERR_ARG, "cp_debug_conv: kind 3 needs slabs");
    if (k >= 3 && (!d->fold || !d->dw)) return fail(CP_ERR_ARG, "cp_debug_conv: kinds 3 and 4 need fold and dw");
    if (k == 4 && !d->db) return fail(CP_ERR_ARG, "cp_debug_conv: kind 4 needs db");
    if (k == 3 && d->gcols && d->gcol_rows <= 0) return fail(CP_ERR_ARG, "cp_debug_conv: gcol_rows must be positive with gcols");
    if (d->gin_exp) {
        if (k < 3 || d->dtype != CP_BF16) return fail(CP_ERR_ARG, "cp_debug_conv: an e5m2 gradient belongs to kinds 3 and 4 under CP_BF16");
        if (k == 3 && !d->gcols) return fail(CP_ERR_ARG, "cp_debug_conv: an e5m2 gradient needs its column sums (gcols)");
    }
    // The conv kernels, colsum_kernel and reduce_rows_kernel index rows in 64 bits, so nothing here wraps at 2^32; the entry still
    // stops where the step does (check_cfg): beyond that no caller of the step has ever run them
    const uint64_t es = d->dtype == CP_F32 ? 4 : 2;
    if ((uint64_t)d->n_windows * 768 * es >= 0xFFF00000ull) return fail(CP_ERR_ARG, "cp_debug_conv: n_windows * 768 * sizeof(T) must stay below 2^32 - 2^20");
    if ((((uintptr_t)d->x | (uintptr_t)d->gin | (uintptr_t)d->gcols | (uintptr_t)d->wc | (uintptr_t)d->out | (uintptr_t)d->partials |
          (uintptr_t)d->slabs | (uintptr_t)d->fold) & 15) != 0)
        return fail(CP_ERR_ARG, "cp_debug_conv: x, gin, gcols, wc, out, partials, slabs and fold must be 16-byte aligned");
    return 0;
}

extern "C" int cp_debug_conv(const cp_debug_conv_args* args, void* stream) {
    if (int e = check_debug_conv(args)) return e;
    if (args->dtype == CP_BF16) return debug_conv_t<bf16_t>(args, (hipStream_t)stream);
    return debug_conv_t<float>(args, (hipStream_t)stream);
}

// One launch sequence of the 512 -> 16 projection on caller buffers, through the launch functions of the step
// (csrc/encoder_api.cuh, gemm_ws.cuh: their row splits, grids and partial-row counts), at any row count
template <typename T>
static int debug_proj_t(const cp_debug_proj_args* d, hipStream_t st) {
    const ProjLaunch pl{st, d->M, d->partials};
    const T* dz = (const T*)d->dz;
    const int* r_exp = (const int*)d->r_exp;
    ProjDrop dp{};
    dp.dp_thresh = d->dp_thresh; dp.dp_key = d->dp_key; dp.dp_inv_keep = d->dp_inv_keep;
    const bool drop = dp.dp_thresh != 0;
    int rows = 0;
    switch (d->kind) {
    case 0:
        if (drop && !r_exp) {
            // (encoder_forward_t: the copy is one job of the batched launch at the start of the pass)
            FoldBatch fb{};
            fb.job[0] = FoldJob{d->Wp, nullptr, d->w32, d->blast, CP_D_E, 512, 32};
            hipLaunchKernelGGL((fold_copy_batch_kernel<T>), dim3(32, 1), dim3(256), 0, st, fb);
            CKL("fold_copy_batch_kernel(last)");
        } else {
            launch_proj_fold<T>(d->Wp, drop ? (const float*)nullptr : d->scale, drop ? (const float*)nullptr : d->shift, d->w32, d->blast, st);
            CKL("fold_linear_kernel(last)");
        }
        if (int e = launch_proj_fwd<T>(pl, d->act, r_exp, d->w32, d->blast, d->scale, d->shift, dp, (float*)d->out)) return e;
        break;
    case 1:
        if (int e = proj_dz_sums<T>(pl, dz, d->dzsum)) return e;
        if (int e = launch_proj_wgrad_tn<T>(pl, st, dz, d->act, r_exp, d->slabs, nullptr, nullptr, dp, d->scale, d->shift, d->dzsum, (float*)d->out,
                                            d->praw, &rows)) return e;
        if (int e = proj_sums_from_wgrad(pl, d->Wp, d->praw, d->dzsum)) return e;
        break;
    case 2:
        if (int e = launch_proj_wgrad_tn<T>(pl, st, dz, d->act, nullptr, d->slabs, d->scale, d->shift, dp, nullptr, nullptr, nullptr, (float*)d->out,
                                            nullptr, &rows)) return e;
        break;
    default:
        if constexpr (sizeof(T) == 2) {
            if (d->kind == 3) {
                if (int e = launch_proj_wgrad_onepass(pl, dz, d->act, r_exp, d->slabs, dp, d->scale, d->shift, d->Wp, (float*)d->out, &rows)) return e;
            } else {
                launch_proj_transpose<T>(d->Wp, d->w32, st);
                CKL("transpose_w_kernel(last)");
                GemmNTArgs a{};
                a.A = dz; a.lda = 64; a.M = d->M; a.K = 64;
                a.W = d->w32; a.F = 512;
                a.C = d->out; a.ldc = 512; a.R = d->act; a.ldr = 512; a.partials = d->partials;
                a.dp_thresh = dp.dp_thresh; a.dp_key = dp.dp_key; a.dp_inv_keep = dp.dp_inv_keep;
                a.coef = d->coef; a.coef_mod = 512;
                CK(launch_proj_dgrad(a, st, &rows));
            }
        }
        break;
    }
    if (d->rows_out) *d->rows_out = rows;
    return 0;
}

// everything a launcher would refuse, or a kernel would read or write out of bounds, before anything launches
static int check_debug_proj(const cp_debug_proj_args* d) {
    if (!d) return fail(CP_ERR_ARG, "cp_debug_proj args");
    if (d->dtype != CP_F32 && d->dtype != CP_BF16) return fail(CP_ERR_ARG, "cp_debug_proj: dtype must be CP_F32 or CP_BF16");
    if (d->kind < 0 || d->kind > 4) return fail(CP_ERR_ARG, "cp_debug_proj: kind must be 0..4");
    if (d->M <= 0) return fail(CP_ERR_ARG, "cp_debug_proj: M must be positive");
    const int k = d->kind;
    const bool b16 = d->dtype == CP_BF16;
    if (k >= 3 && !b16) return fail(CP_ERR_ARG, "cp_debug_proj: kinds 3 and 4 belong to CP_BF16");
    if (d->r_exp && (!b16 || k == 2 || k == 4)) return fail(CP_ERR_ARG, "cp_debug_proj: an e4m3 activation (r_exp) belongs to kinds 0, 1 and 3 under CP_BF16");
    if (!d->Wp || !d->act || !d->out) return fail(CP_ERR_ARG, "cp_debug_proj: Wp, act and out must not be NULL");
    if (k != 0 && !d->dz) return fail(CP_ERR_ARG, "cp_debug_proj: dz must not be NULL");
    if (k != 4 && (!d->scale || !d->shift)) return fail(CP_ERR_ARG, "cp_debug_proj: kinds 0..3 need scale and shift");
    if (k == 4 && !d->coef) return fail(CP_ERR_ARG, "cp_debug_proj: kind 4 needs coef");
    if ((k == 0 || k == 4) && !d->w32) return fail(CP_ERR_ARG, "cp_debug_proj: kinds 0 and 4 need w32");
    if (k == 0 && !d->blast) return fail(CP_ERR_ARG, "cp_debug_proj: the forward needs blast");
    if (k >= 1 && k <= 3 && !d->slabs) return fail(CP_ERR_ARG, "cp_debug_proj: kinds 1..3 need slabs");
    if ((k == 1 || k >= 3) && !d->partials) return fail(CP_ERR_ARG, "cp_debug_proj: kinds 1, 3 and 4 need partials");
    if (k == 1 && (!d->praw || !d->dzsum)) return fail(CP_ERR_ARG, "cp_debug_proj: kind 1 needs praw and dzsum");
    const bool drop = d->dp_thresh != 0;
    if (k == 1 && (drop || d->dp_key != 0 || d->dp_inv_keep != 0.f)) return fail(CP_ERR_ARG, "cp_debug_proj: kind 1 takes no dropout");
    if (k >= 2 && !drop) return fail(CP_ERR_ARG, "cp_debug_proj: kinds 2..4 run behind a dropout (dp_thresh != 0)");
    if (!drop && (d->dp_key != 0 || d->dp_inv_keep != 0.f)) return fail(CP_ERR_ARG, "cp_debug_proj: dp_key and dp_inv_keep without dp_thresh");
    if (drop && (d->dp_thresh > 65535u || !(d->dp_inv_keep > 0.f))) return fail(CP_ERR_ARG, "cp_debug_proj: dp_thresh in 1..65535, dp_inv_keep > 0");
    // 32-bit byte offsets of the buffer loads and stores and the dropout hash's 32-bit element index (check_cfg)
    const uint64_t es = b16 ? 2 : 4;
    // (by division: no M wraps the product)
    if ((uint64_t)d->M >= (0xFFF00000ull + 512 * es - 1) / (512 * es)) return fail(CP_ERR_ARG, "cp_debug_proj: M * 512 * sizeof(T) must stay below 2^32 - 2^20");
    if ((((uintptr_t)d->Wp | (uintptr_t)d->act | (uintptr_t)d->dz | (uintptr_t)d->w32 | (uintptr_t)d->out | (uintptr_t)d->slabs |
          (uintptr_t)d->partials | (uintptr_t)d->praw | (uintptr_t)d->scale | (uintptr_t)d->shift | (uintptr_t)d->coef | (uintptr_t)d->blast |
          (uintptr_t)d->dzsum) & 15) != 0)
        return fail(CP_ERR_ARG, "cp_debug_proj: Wp, act, dz, w32, out, slabs, partials, praw, scale, shift, coef, blast and dzsum must be 16-byte aligned");
    return 0;
}

extern "C" int cp_debug_proj(const cp_debug_proj_args* args, void* stream) {
    if (int e = check_debug_proj(args)) return e;
    if (args->dtype == CP_BF16) return debug_proj_t<bf16_t>(args, (hipStream_t)stream);
    return debug_proj_t<float>(args, (hipStream_t)stream);
}

// One launch sequence of the 8-bit fc path on caller buffers and a caller scale table, through the launch functions of the step
// (csrc/fp8.cuh, csrc/encoder_api.cuh: their grids, row splits and partial-row counts), at any row count
static int debug_fp8(const cp_debug_fp8_args* d, hipStream_t st) {
    Fp8State* fs = (Fp8State*)d->state;
    const int64_t M = d->M;
    int rows = 0;
    switch (d->kind) {
    case 0: {
        Ws8Args a{};
        a.A = (const uint8_t*)d->A; a.W = (const uint8_t*)d->W; a.wsc = (const uint8_t*)d->wsc; a.bias = d->bias; a.C = (uint8_t*)d->C;
        a.partials = d->partials; a.amax = &fs->amax[d->t_out]; a.M = M; a.F = d->F;
        if (d->K == 512) CK(launch_gemm_ws8<512>(a, st, &rows));
        else CK(launch_gemm_ws8<768>(a, st, &rows));
        if (!d->partials) rows = 0;
        break;
    }
    case 1:
    case 2: {
        Wsd8Args a{};
        a.A = (const uint8_t*)d->A; a.W = (const uint8_t*)d->W; a.wsc = (const uint8_t*)d->wsc; a.R = (const uint8_t*)d->R; a.C = d->C;
        a.partials = d->partials; a.st = fs; a.t_r = d->t_r; a.t_out = d->t_out; a.M = M; a.F = d->F;
        if (d->kind == 1) {
            a.coef = d->coef; a.coef_mod = d->coef_mod;
            CK((launch_gemm_wsd8<0>(a, st, &rows)));
        } else {
            a.bn_stats = d->bn_stats; a.dp_inv_keep = d->dp_inv_keep;
            CK((launch_gemm_wsd8<1>(a, st, &rows)));
        }
        break;
    }
    case 3: {
        const bool paired = d->mode == 1;
        GemmTN8Args ta{};
        ta.X = (const uint8_t*)d->A; ta.ldx = 512; ta.Y = (const uint8_t*)d->R; ta.ldy = d->F; ta.slabs = d->partials; ta.M = M; ta.P = 512; ta.Q = d->F;
        split_rows_tn8(M, paired, d->F, &rows, &ta.rows_per_split);
        if (paired) { ta.X2 = (const uint8_t*)d->A2; ta.Y2 = (const uint8_t*)d->R2; ta.slabs2 = d->partials2; }
        ta.splits = rows;
        CK(launch_gemm_tn8(ta, st));
        if (paired) launch_reduce_slabs8(d->partials2, rows, 512, nullptr, nullptr, nullptr, d->C2, 0, nullptr, (const int*)&fs->e[d->t_in2], (const int*)&fs->e[d->t_r2], st);
        launch_reduce_slabs8(d->partials, rows, d->F, nullptr, nullptr, nullptr, (float*)d->C, 0, nullptr, (const int*)&fs->e[d->t_in], (const int*)&fs->e[d->t_r], st);
        CKL("reduce_slabs_kernel<bf16>");
        break;
    }
    case 4:
        launch_bn_dropout_apply8((const uint8_t*)d->A, d->bn_stats, (uint8_t*)d->C, M, d->dp_thresh, d->dp_key, d->dp_inv_keep, nullptr, fs, d->t_in, d->t_out, st);
        CKL("bn_dropout_apply8_kernel");
        break;
    case 5:
        rows = launch_bn_relu_bwd8((uint8_t*)d->C, (const uint8_t*)d->R, d->coef, d->partials, M, fs, d->t_in, d->t_r, d->t_out, st);
        CKL("bn_relu_bwd8_kernel");
        break;
    case 6: {
        Proj8Args a{};
        a.A = (const bf16_t*)d->A; a.lda = 64; a.W = (const bf16_t*)d->W; a.K = 64; a.R = (const uint8_t*)d->R; a.C = (uint8_t*)d->C;
        a.partials = d->partials; a.coef = d->coef; a.st = fs; a.t_r = d->t_r; a.t_out = d->t_out; a.M = M;
        a.dp_thresh = d->dp_thresh; a.dp_key = d->dp_key; a.dp_inv_keep = d->dp_inv_keep;
        CK(launch_proj_dgrad8(a, st, &rows));
        break;
    }
    case 7:
        if (d->mode < 2) {
            launch_fold_linear8((const float*)d->A, d->bias, d->scale, d->shift, (uint8_t*)d->C, (uint8_t*)d->wsc, d->partials, d->K, d->mode, fs,
                                d->t_in, d->t_out, st);
            CKL("fold_linear8_kernel");
        } else {
            Transpose8Batch tb{};
            tb.job[0] = Transpose8Job{(const float*)d->A, (uint8_t*)d->C, (uint8_t*)d->wsc, d->K, d->mode == 3 ? 1 : 0, d->t_in};
            launch_transpose_w8_batch(tb, 1, fs, st);
            CKL("transpose_w8_batch_kernel");
        }
        break;
    default:
        hipLaunchKernelGGL(fp8_update_scales_kernel, dim3(1), dim3(64), 0, st, fs, M);
        CKL("fp8_update_scales_kernel");
        break;
    }
    if (d->rows_out) *d->rows_out = rows;
    return 0;
}

// everything a launcher would refuse, or a kernel would read or write out of bounds, before anything launches
static int check_debug_fp8(const cp_debug_fp8_args* d) {
    if (!d) return fail(CP_ERR_ARG, "cp_debug_fp8 args");
    if (d->kind < 0 || d->kind > 8) return fail(CP_ERR_ARG, "cp_debug_fp8: kind must be 0..8");
    const int k = d->kind;
    if (!d->state) return fail(CP_ERR_ARG, "cp_debug_fp8: state must not be NULL");
    if (d->M <= 0) return fail(CP_ERR_ARG, "cp_debug_fp8: M must be positive");
    if ((k == 3 && d->mode != 0 && d->mode != 1) || (k == 7 && (d->mode < 0 || d->mode > 3)) || (k != 3 && k != 7 && d->mode != 0))
        return fail(CP_ERR_ARG, "cp_debug_fp8: mode must be 0 | 1 in kind 3, 0..3 in kind 7, else 0");
    const bool paired = k == 3 && d->mode == 1;
    if (k != 8) {
        if ((k != 5 && !d->A) || !d->C) return fail(CP_ERR_ARG, "cp_debug_fp8: A and C must not be NULL");
        if (k != 0 && k != 4 && !(k == 7 && d->mode >= 2) && !d->partials) return fail(CP_ERR_ARG, "cp_debug_fp8: partials must not be NULL");
        if ((k <= 2 || k == 6) && !d->W) return fail(CP_ERR_ARG, "cp_debug_fp8: W must not be NULL");
        if ((k <= 2 || k == 7) && !d->wsc) return fail(CP_ERR_ARG, "cp_debug_fp8: wsc must not be NULL");
        if (k == 0 && !d->bias) return fail(CP_ERR_ARG, "cp_debug_fp8: the forward needs a bias");
        if ((k == 1 || k == 2 || k == 3 || k == 5 || k == 6) && !d->R) return fail(CP_ERR_ARG, "cp_debug_fp8: R must not be NULL");
        if ((k == 1 || k == 5 || k == 6) && !d->coef) return fail(CP_ERR_ARG, "cp_debug_fp8: kinds 1, 5 and 6 need coef");
        if ((k == 2 || k == 4) && !d->bn_stats) return fail(CP_ERR_ARG, "cp_debug_fp8: kinds 2 and 4 need bn_stats");
        if (paired && (!d->A2 || !d->R2 || !d->partials2 || !d->C2)) return fail(CP_ERR_ARG, "cp_debug_fp8: a paired launch needs A2, R2, partials2 and C2");
        if (k == 7 && d->mode < 2 && !d->scale != !d->shift) return fail(CP_ERR_ARG, "cp_debug_fp8: scale and shift come together");
    }
    // shapes the launch functions refuse or the kernels are not written for
    if (k == 0 && ((d->K != 512 && d->K != 768) || d->F != 512)) return fail(CP_ERR_ARG, "cp_debug_fp8: kind 0 takes K = 512 | 768 and F = 512");
    if ((k == 1 || k == 3) && d->F != 512 && d->F != 768) return fail(CP_ERR_ARG, "cp_debug_fp8: kinds 1 and 3 take F = 512 | 768");
    if ((k == 2 || (k >= 4 && k <= 6) || paired) && d->F != 512) return fail(CP_ERR_ARG, "cp_debug_fp8: kinds 2, 4, 5, 6 and a paired launch take F = 512");
    if (k == 7 && d->K != 512 && d->K != 768) return fail(CP_ERR_ARG, "cp_debug_fp8: kind 7 takes K = 512 | 768");
    if (k == 1 && d->coef_mod <= 0) return fail(CP_ERR_ARG, "cp_debug_fp8: coef_mod must be positive");
    // scale-table ids
    auto id_ok = [](int t) { return t >= 0 && t < F8_NT; };
    if ((k == 3 || k == 4 || k == 5 || k == 7) && !id_ok(d->t_in)) return fail(CP_ERR_ARG, "cp_debug_fp8: t_in outside 0..63");
    if (((k >= 1 && k <= 3) || k == 5 || k == 6) && !id_ok(d->t_r)) return fail(CP_ERR_ARG, "cp_debug_fp8: t_r outside 0..63");
    if ((k <= 2 || (k >= 4 && k <= 6)) && !id_ok(d->t_out)) return fail(CP_ERR_ARG, "cp_debug_fp8: t_out outside 0..63");
    if (k == 7 && d->mode < 2 && !(id_ok(d->t_out) || d->t_out == -1)) return fail(CP_ERR_ARG, "cp_debug_fp8: t_out outside -1..63");
    if (paired && (!id_ok(d->t_in2) || !id_ok(d->t_r2))) return fail(CP_ERR_ARG, "cp_debug_fp8: t_in2 and t_r2 outside 0..63");
    // dropout
    if (d->dp_thresh > 65535u) return fail(CP_ERR_ARG, "cp_debug_fp8: dp_thresh must not exceed 65535");
    if ((k == 2 || k == 4 || (k == 6 && d->dp_thresh != 0)) && !(d->dp_inv_keep > 0.f)) return fail(CP_ERR_ARG, "cp_debug_fp8: dp_inv_keep must be positive");
    // 32-bit byte offsets of the buffer loads and stores, the "no such tile" offset 0xFFF00000 and the hash's 32-bit element index
    if (k <= 6) {
        const int kk = k == 0 ? d->K : 512, wide = kk > d->F ? kk : d->F;
        if ((uint64_t)d->M >= (0xFFF00000ull + wide - 1) / wide) return fail(CP_ERR_ARG, "cp_debug_fp8: M * max(K, F) must stay below 2^32 - 2^20");
    }
    if ((((uintptr_t)d->state | (uintptr_t)d->A | (uintptr_t)d->W | (uintptr_t)d->wsc | (uintptr_t)d->bias | (uintptr_t)d->R | (uintptr_t)d->coef |
          (uintptr_t)d->bn_stats | (uintptr_t)d->scale | (uintptr_t)d->shift | (uintptr_t)d->C | (uintptr_t)d->partials | (uintptr_t)d->A2 |
          (uintptr_t)d->R2 | (uintptr_t)d->partials2 | (uintptr_t)d->C2) & 15) != 0)
        return fail(CP_ERR_ARG, "cp_debug_fp8: state, A, W, wsc, bias, R, coef, bn_stats, scale, shift, C, partials, A2, R2, partials2 and C2 must be 16-byte aligned");
    return 0;
}

extern "C" int cp_debug_fp8(const cp_debug_fp8_args* args, void* stream) {
    if (int e = check_debug_fp8(args)) return e;
    return debug_fp8(args, (hipStream_t)stream);
}

// One f32 / bf16 BatchNorm or weight-preparation launch sequence of the large-batch step on caller buffers, through the launch
// functions of the step (csrc/encoder_api.cuh: their grids, caps, job tables and the pre-reduce rule), at any row count
template <typename T>
static int debug_bn_t(const cp_debug_bn_args* d, hipStream_t st) {
    const PreReduce pre{d->kind == 4 ? d->partials : d->rows, d->scratch, st};
    PrepImages im{};
    for (int i = 0; i < CP_N_FC; ++i) { im.wfc[i] = d->wimg[i]; im.bfc[i] = d->bimg[i]; im.wfc_t[i] = d->wimg[i]; }
    im.wlast = d->wimg[CP_N_FC]; im.blast = d->bimg[CP_N_FC]; im.wlast_t = d->wimg[CP_N_FC];
    int rows = 0;
    switch (d->kind) {
    case 0: {
        int nrows = (int)d->M;
        const float* pp = pre(nrows, 2 * d->C);
        launch_bn_finalize(pp, nrows, d->count, d->gamma, d->beta, d->running_mean, d->running_var, d->update_running ? 1 : 0, d->momentum, d->eps,
                           d->stats, d->C, (const int*)d->unscale_exp, st);
        CKL("bn_finalize_kernel");
        break;
    }
    case 1: {
        StatsTables tb{};
        for (int l = 0; l < CP_N_BN; ++l) tb.t[l] = d->stats9[l];
        launch_running_stats(d->params, d->bn, tb, d->eps, st);
        CKL("bn_running_stats_kernel");
        launch_eval_folds<T>(d->params, tb, im, st);
        CKL("fold_linear_batch_kernel");
        break;
    }
    case 2: {
        int nr = (int)d->M;
        const float* pp = pre(nr, 2 * d->C * d->nfold);
        launch_bn_bwd_finalize(pp, nr, d->count, d->stats, d->coef, d->dgamma, d->dbeta, d->C, d->nfold, d->local, st);
        CKL("bn_bwd_finalize_kernel");
        break;
    }
    case 3:
        launch_bn_dropout_apply<T>((const T*)d->r, d->stats, (T*)d->g, d->M, d->dp_thresh, d->dp_key, d->dp_inv_keep, nullptr, st);
        CKL("bn_dropout_apply_kernel");
        break;
    case 4:
        rows = launch_bn_relu_bwd<T>((T*)d->g, (const T*)d->r, d->coef, d->partials, d->M, d->C, d->C == 512 ? CAP_BRB16 : 2048, st);
        launch_bias_grad_from_rows(pre, rows, d->C, d->db);
        CKL("bn_relu_bwd_kernel");
        break;
    default:
        if (d->mode <= 1) {
            launch_fold_linear<T>(d->W, d->b, d->s, d->t, d->wimg[0], d->bimg[0], d->K, d->mode, st);
            CKL("fold_linear_kernel");
        } else if (d->mode == 2) {
            launch_fold_copies<T>(d->params, im, st);
            CKL("fold_copy_batch_kernel");
        } else {
            if (int e = launch_weight_transposes<T>(d->params, im, st)) return e;
        }
        break;
    }
    if (d->rows_out) *d->rows_out = rows;
    return 0;
}

// everything a launch function would be handed blindly, or a kernel would read or write out of bounds, before anything launches
static int check_debug_bn(const cp_debug_bn_args* d) {
    if (!d) return fail(CP_ERR_ARG, "cp_debug_bn args");
    if (d->dtype != CP_F32 && d->dtype != CP_BF16) return fail(CP_ERR_ARG, "cp_debug_bn: dtype must be CP_F32 or CP_BF16");
    if (d->kind < 0 || d->kind > 5) return fail(CP_ERR_ARG, "cp_debug_bn: kind must be 0..5");
    const int k = d->kind;
    if (d->mode < 0 || d->mode > (k == 5 ? 3 : 0)) return fail(CP_ERR_ARG, "cp_debug_bn: mode must be 0..3 in kind 5, else 0");
    const bool rowed = k == 0 || k == 2 || k == 3 || k == 4;
    if (rowed && d->M <= 0) return fail(CP_ERR_ARG, "cp_debug_bn: M must be positive");
    if ((k == 0 || k == 2 || k == 4) && d->C != 64 && d->C != 512) return fail(CP_ERR_ARG, "cp_debug_bn: C must be 64 or 512");
    if (k == 2 && !(d->nfold == 1 || (d->nfold == 12 && d->C == 64))) return fail(CP_ERR_ARG, "cp_debug_bn: (C, nfold) must be (512, 1), (64, 1) or (64, 12)");
    if (k == 5 && d->mode <= 1 && !(d->K == 768 || (d->K == 512 && d->mode == 0))) return fail(CP_ERR_ARG, "cp_debug_bn: K must be 512 or 768 in mode 0, 768 in mode 1");
    if ((k == 0 || k == 2) && !(d->count >= 1.0)) return fail(CP_ERR_ARG, "cp_debug_bn: count must be at least 1");
    if ((k == 0 || k == 2) && d->M >= (1ll << 31)) return fail(CP_ERR_ARG, "cp_debug_bn: M must stay below 2^31 partial rows");
    uintptr_t al = 0;          // every pointer the kind hands on, for the alignment check
    auto need = [&](const void* p) { al |= (uintptr_t)p; return p != nullptr; };
    auto opt_ = [&](const void* p) { al |= (uintptr_t)p; };
    if (k == 0) {
        if (!need(d->rows) || !need(d->gamma) || !need(d->beta) || !need(d->scratch) || !need(d->stats))
            return fail(CP_ERR_ARG, "cp_debug_bn: kind 0 needs rows, gamma, beta, scratch and stats");
        if (!d->running_mean != !d->running_var) return fail(CP_ERR_ARG, "cp_debug_bn: running_mean and running_var come together");
        if (d->update_running && !d->running_mean) return fail(CP_ERR_ARG, "cp_debug_bn: update_running without running buffers");
        opt_(d->running_mean); opt_(d->running_var);
        if ((uintptr_t)d->unscale_exp & 3) return fail(CP_ERR_ARG, "cp_debug_bn: unscale_exp must be 4-byte aligned");
    }
    if (k == 1 || (k == 5 && d->mode >= 2)) {
        const cp_params* p = d->params;
        if (!p) return fail(CP_ERR_ARG, "cp_debug_bn: params must not be NULL");
        const int first = (k == 5 && d->mode == 2) ? 4 : 0;
        for (int i = first; i < CP_N_FC; ++i)
            if (!need(p->fc_w[i]) || !need(d->wimg[i]) || (!(k == 5 && d->mode == 3) && (!need(p->fc_b[i]) || !need(d->bimg[i]))))
                return fail(CP_ERR_ARG, "cp_debug_bn: params->fc_w, params->fc_b, wimg and bimg of every layer the launch prepares must not be NULL");
        if (!need(p->last_w) || !need(d->wimg[CP_N_FC]) || (!(k == 5 && d->mode == 3) && !need(d->bimg[CP_N_FC])))
            return fail(CP_ERR_ARG, "cp_debug_bn: params->last_w, wimg[7] and bimg[7] must not be NULL");
    }
    if (k == 1) {
        if (!d->bn) return fail(CP_ERR_ARG, "cp_debug_bn: bn must not be NULL");
        for (int l = 0; l < CP_N_BN; ++l)
            if (!need(d->params->bn_g[l]) || !need(d->params->bn_b[l]) || !need(d->bn->running_mean[l]) || !need(d->bn->running_var[l]) || !need(d->stats9[l]))
                return fail(CP_ERR_ARG, "cp_debug_bn: kind 1 needs nine bn_g, bn_b, running_mean, running_var and stats9 tables");
    }
    if (k == 2) {
        if (!need(d->rows) || !need(d->scratch) || !need(d->stats) || !need(d->coef) || !need(d->dgamma) || !need(d->dbeta))
            return fail(CP_ERR_ARG, "cp_debug_bn: kind 2 needs rows, scratch, stats, coef, dgamma and dbeta");
        opt_(d->local);
    }
    if (k == 3) {
        if (!need(d->r) || !need(d->stats) || !need(d->g)) return fail(CP_ERR_ARG, "cp_debug_bn: kind 3 needs r, stats and g");
        if (d->dp_thresh > 65535u || !(d->dp_inv_keep > 0.f)) return fail(CP_ERR_ARG, "cp_debug_bn: dp_thresh must not exceed 65535, dp_inv_keep must be positive");
    }
    if (k == 4 && (!need(d->r) || !need(d->g) || !need(d->coef) || !need(d->partials) || !need(d->scratch) || !need(d->db)))
        return fail(CP_ERR_ARG, "cp_debug_bn: kind 4 needs r, g, coef, partials, scratch and db");
    if (k == 5 && d->mode <= 1) {
        if (!need(d->W) || !need(d->b) || !need(d->wimg[0]) || !need(d->bimg[0])) return fail(CP_ERR_ARG, "cp_debug_bn: modes 0 and 1 need W, b, wimg[0] and bimg[0]");
        if (!d->s != !d->t) return fail(CP_ERR_ARG, "cp_debug_bn: s and t come together");
        opt_(d->s); opt_(d->t);
    }
    if (k == 3 || k == 4) {
        // 32-bit byte offsets of the buffer loads and stores and the dropout hash's 32-bit element index (check_cfg); by division: no M wraps
        const uint64_t rowb = (uint64_t)(k == 3 ? 512 : d->C) * (d->dtype == CP_BF16 ? 2 : 4);
        if ((uint64_t)d->M >= (0xFFF00000ull + rowb - 1) / rowb) return fail(CP_ERR_ARG, "cp_debug_bn: M * C * sizeof(T) must stay below 2^32 - 2^20");
    }
    if ((al & 15) != 0) return fail(CP_ERR_ARG, "cp_debug_bn: every buffer must be 16-byte aligned");
    return 0;
}

extern "C" int cp_debug_bn(const cp_debug_bn_args* args, void* stream) {
    if (int e = check_debug_bn(args)) return e;
    if (args->dtype == CP_BF16) return debug_bn_t<bf16_t>(args, (hipStream_t)stream);
    return debug_bn_t<float>(args, (hipStream_t)stream);
}

__global__ __launch_bounds__(256) void hog_kernel(long long ticks, float* sink) {
    __shared__ float pad[30 * 1024];                       // 120 KiB: no 64 KiB-stage GEMM block fits beside this one
    pad[threadIdx.x] = (float)threadIdx.x;
    const long long t0 = __builtin_amdgcn_s_memrealtime();           // 100 MHz
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
    if (sink && pad[threadIdx.x] < -1.f) *sink = pad[0];
}
extern "C" int cp_debug_hog(int32_t blocks, int32_t microseconds, void* stream) {
    if (blocks <= 0 || microseconds <= 0 || microseconds > 100000) return fail(CP_ERR_ARG, "cp_debug_hog args");
    hipLaunchKernelGGL(hog_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (long long)microseconds * 100, (float*)nullptr);
    CKL("hog_kernel");
    return 0;
}

extern "C" int cp_debug_gemm(int32_t dtype, int32_t kind, int64_t M, int32_t K, int32_t F, const void* A, const void* W,
                             void* C, const float* bias, const void* R, float* partials, void* stream) {
    if (!A || !W || !C || !partials || M <= 0 || K % 64 || F % 256 || kind < 0 || kind > 2)
        return fail(CP_ERR_ARG, "cp_debug_gemm args");
    // the static schedule, no coefficients, no dropout.  (R and bias are read by the kinds that have them.)
    cp_debug_fc_gemm_args d{};
    d.dtype = dtype == CP_BF16 ? CP_BF16 : CP_F32; d.kind = kind; d.M = M; d.K = K; d.F = F; d.tile_schedule = CP_TILES_STATIC;
    d.A = A; d.W = W; d.C = C; d.bias = kind == 0 ? bias : nullptr; d.R = kind == 1 ? R : nullptr; d.partials = partials;
    return cp_debug_fc_gemm(&d, stream);
}

#include "online_api.cuh"             // the cp_online_* entries: host layer of the online decoders, the gate, the gate sweep and the subset sweep
