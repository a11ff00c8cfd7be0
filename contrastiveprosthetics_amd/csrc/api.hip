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
#include "online_gate.cuh"

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
// workspace layout
// ---------------------------------------------------------------------------------------
static const int kLayerC[CP_N_BN] = {64, 64, 512, 512, 512, 512, 512, 512, 512};
static inline int fcK(int i) { return i == 0 ? 768 : 512; }
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct WS {
    size_t act[CP_N_BN];     // post-ReLU outputs, T
    size_t u[4];             // dropout(BN(.)) of fc4..fc7, T (only when dp > 0)
    size_t gbuf[2];          // gradient ping-pong, T [N][768]
    size_t dz;               // [N][64] T
    size_t partials;         // f32
    size_t partials2;        // f32 [REDUCE_SLICES][<=2048]: pre-reduced partial rows
    size_t stats[CP_N_BN];   // [4][C] f32
    size_t coef;             // [3][512] f32
    size_t wc2_f, wc2_d;     // conv2 weights, T [64][192]
    size_t wfc[CP_N_FC], bfc[CP_N_FC], wfc_t[CP_N_FC];
    size_t wlast, blast, wlast_t, dzsum;
    size_t slabs;            // f32
    size_t praw;             // f32 [512][768]: raw (un-fixed) weight-gradient product of the current layer
    size_t head_part;        // f32
    size_t sm_acc;                // i64 [18][2][768]: fixed-point BatchNorm totals of the small-batch form (csrc/small.cuh): forward layers 0..8, backward 9..17
    size_t sync_loc, sync_glob;   // f32 [2][768] each: one row of statistics, this rank's and the sum over ranks (sync BN)
    // second stream (cp_config.aux_stream): gradients that a floating weight-gradient launch still reads must outlive the ping-pong --
    // gkeep[q] = dL/d(pre-activation) of fc7, fc6, fc5 (T [N][512]; CP_FP8: e5m2 bytes); slabs_b = that stream's own slab region
    size_t gkeep[3], slabs_b;
    // CP_FP8 (csrc/fp8.cuh): the scale table (ALWAYS at offset 0, so that it survives a change of n_windows), the e4m3 activations,
    // dropout outputs and fc weights with their scale bytes; the 16-bit buffers above are then what the bf16 backward kernels read
    size_t f8state, act8[CP_N_BN], u8[3], wfc8[CP_N_FC], wsc8[CP_N_FC];
    size_t g8[2], wfc8t[CP_N_FC], wsc8t[CP_N_FC];      // backward: e5m2 gradient ping-pong [N][512], W^T as e4m3 [K][512] + scale bytes [K]
    size_t total;
    size_t partials_floats, slabs_floats;
};
static const size_t kSlabFloats = (size_t)64 * 512 * 512 + 1024;   // 64 splits of a 512x512 (or 40 of a 512x768) f32 slab
static const int kHeadBlocksMax = 1024;          // (512 / 256 measured: 44.4 / 54.1 us against 43.6)
static const int kSumSlices = 16;           // row slices (= partial rows) of bn_bwd_sums_from_wgrad_kernel
static const int kProjSplits = 128;         // row splits of the projection's weight-gradient launch

static WS carve(int64_t N, int dtype, float dp) {
    WS w{};
    const size_t es = dtype == CP_F32 ? 4 : 2;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align256(o + bytes); return r; };
    if (dtype == CP_FP8) {
        w.f8state = take(F8_STATE_BYTES);
        for (int l = 1; l < CP_N_BN; ++l) w.act8[l] = take((size_t)N * (l < 2 ? 768 : 512));
        for (int i = 0; i < 3; ++i) w.u8[i] = dp > 0.f ? take((size_t)N * 512) : 0;
        for (int i = 0; i < CP_N_FC; ++i) {
            w.wfc8[i] = take((size_t)512 * fcK(i));
            w.wsc8[i] = take(512);
            w.wfc8t[i] = take((size_t)512 * fcK(i));
            w.wsc8t[i] = take(768);
        }
        for (int i = 0; i < 2; ++i) w.g8[i] = take((size_t)N * 512);
    }
    // (conv1's output is never stored: act[0] is empty, its consumers recompute it from x)
    for (int l = 0; l < CP_N_BN; ++l) w.act[l] = take(l == 0 ? 0 : (size_t)N * (l < 2 ? 768 : 512) * es);
    for (int i = 0; i < 4; ++i) w.u[i] = dp > 0.f ? take((size_t)N * 512 * es) : 0;
    for (int i = 0; i < 2; ++i) w.gbuf[i] = take((size_t)N * 768 * es);
    w.dz = take((size_t)N * 64 * es);
    w.partials_floats = (size_t)12 * N + 4 * 1024 * 1024;
    w.partials = take(w.partials_floats * 4);
    w.partials2 = take((size_t)REDUCE_SLICES * 2048 * 4);
    for (int l = 0; l < CP_N_BN; ++l) w.stats[l] = take(4 * 512 * 4);
    w.coef = take(3 * 512 * 4);
    w.wc2_f = take(64 * 192 * es);
    w.wc2_d = take(64 * 192 * es);
    for (int i = 0; i < CP_N_FC; ++i) {
        w.wfc[i] = take((size_t)512 * fcK(i) * es);
        w.bfc[i] = take(512 * 4);
        w.wfc_t[i] = take((size_t)512 * fcK(i) * es);
    }
    w.wlast = take(32 * 512 * es);
    w.blast = take(32 * 4);
    w.wlast_t = take(512 * 64 * es);
    w.dzsum = take(64 * 4);
    w.slabs_floats = kSlabFloats;
    w.slabs = take(kSlabFloats * 4);
    w.praw = take((size_t)512 * 768 * 4);
    w.head_part = take((size_t)kHeadBlocksMax * HEAD_PART * 4);
    w.sm_acc = take((size_t)18 * 2 * 768 * 8);
    w.sync_loc = take(2 * 768 * 4);
    w.sync_glob = take(2 * 768 * 4);
    for (int i = 0; i < 3; ++i) w.gkeep[i] = dp > 0.f ? take((size_t)N * 512 * (dtype == CP_FP8 ? 1 : es)) : 0;
    w.slabs_b = dp > 0.f ? take(kSlabFloats * 4) : 0;
    w.total = o;
    return w;
}

extern "C" size_t cp_workspace_bytes(int64_t max_windows, int32_t dtype, float dp_emg) {
    if (max_windows <= 0) return 0;
    return carve(max_windows, dtype, dp_emg).total;
}

static uint32_t host_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// device cp_step_state of a graph-replayed step (cp_config.step_state_lo/hi), or nullptr
static const uint32_t* dp_salt(const cp_config* c) {
    const uint64_t addr = ((uint64_t)c->step_state_hi << 32) | (uint64_t)c->step_state_lo;
    return (const uint32_t*)(uintptr_t)addr;       // first word of the struct = dp_salt
}
static uint32_t dp_key(const cp_config* c, int layer) {
    const uint64_t step = dp_salt(c) ? 0 : c->step;          // graph mode: the step enters through the device salt
    return host_hash32((uint32_t)c->seed ^ host_hash32((uint32_t)(c->seed >> 32) + 0x51ed27U) ^
                       host_hash32((uint32_t)step * 0x9E3779B1U + (uint32_t)layer * 0x85EBCA77U +
                                   (uint32_t)(step >> 32)));
}
static uint32_t dp_thresh(float p) {
    double t = (double)p * 65536.0 + 0.5;
    if (t < 1.0) t = 1.0;
    if (t > 65535.0) t = 65535.0;
    return (uint32_t)t;
}
static float dp_inv_keep(float p) { return 1.0f / (1.0f - (float)dp_thresh(p) / 65536.0f); }

static int check_cfg(const cp_config* c, void* ws, size_t ws_bytes, WS* out) {
    if (!c || !ws) return fail(CP_ERR_ARG, "null config/workspace");
    if (c->n_windows <= 0 || c->n_windows % CP_TASKS != 0) return fail(CP_ERR_ARG, "n_windows must be a positive multiple of 41");
    if (c->dtype != CP_F32 && c->dtype != CP_BF16 && c->dtype != CP_FP8) return fail(CP_ERR_ARG, "dtype");
    if (c->dp_emg < 0.f || c->dp_emg >= 1.f) return fail(CP_ERR_ARG, "dp_emg");
    if (c->tile_schedule != CP_TILES_STATIC && c->tile_schedule != CP_TILES_DYNAMIC) return fail(CP_ERR_ARG, "tile_schedule");
    if (c->stats_allreduce && c->stats_world < 1) return fail(CP_ERR_ARG, "stats_world");
    // 32-bit byte offsets into an [n_windows][768] 16-bit tensor (the weight-stationary kernels' buffer loads) and the dropout hash's
    // 32-bit element index: 2,795,000 windows = 68,000 groups per call (the 288 GB of HBM hold fewer in f32 anyway)
    if ((uint64_t)c->n_windows * 768 * 2 >= 0xFFF00000ull) return fail(CP_ERR_ARG, "n_windows * 1536 must stay below 2^32 (32-bit buffer offsets)");
    *out = carve(c->n_windows, c->dtype, c->dp_emg);
    if (out->total > ws_bytes) return fail(CP_ERR_WORKSPACE, "workspace too small");
    if (((uintptr_t)ws & 255) != 0) return fail(CP_ERR_ARG, "workspace must be 256-byte aligned");
    return 0;
}

// The second stream of cp_encoder_backward (cp_config.aux_stream; cpnative.h).  fork(): what is on `main` so far precedes what is
// enqueued on `side` from now on; join(): what is on `side` so far precedes what is enqueued on `main` from now on.  One event each, re-recorded:
// a stream's wait refers to the record that precedes it.
struct Aux {
    hipStream_t main, side;
    hipEvent_t fork_ev, join_ev;
    bool on;
    int fork() const {
        if (!on) return 0;
        CK(hipEventRecord(fork_ev, main));
        CK(hipStreamWaitEvent(side, fork_ev, 0));
        return 0;
    }
    int join() const {
        if (!on) return 0;
        CK(hipEventRecord(join_ev, side));
        CK(hipStreamWaitEvent(main, join_ev, 0));
        return 0;
    }
    hipStream_t s() const { return on ? side : main; }
};
static Aux make_aux(const cp_config* c, hipStream_t st, bool eligible) {
    Aux a{st, st, nullptr, nullptr, false};
    if (eligible && c->aux_stream && c->aux_fork && c->aux_join && !c->stats_allreduce && !c->grad_tap) {
        a.side = (hipStream_t)c->aux_stream; a.fork_ev = (hipEvent_t)c->aux_fork; a.join_ev = (hipEvent_t)c->aux_join;
        a.on = a.side != st;
    }
    return a;
}

// the transposed weights the data-gradient launches read: fc1..fc7 and the projection (bf16 / f32), their e4m3 form + the projection's
// (CP_FP8).  Made once per step: at the start of the backward pass, or -- second stream -- beside the forward pass.
template <typename T>
static int launch_weight_transposes(const cp_params* p, unsigned char* base, const WS& w, hipStream_t st) {
    ProfScope ps(CP_K_PREP, st);
    TransposeBatch tb{};
    for (int i = 0; i < CP_N_FC; ++i) tb.job[i] = TransposeJob{p->fc_w[i], base + w.wfc_t[i], 512, fcK(i), 512, i == 0 ? 1 : 0};
    tb.job[CP_N_FC] = TransposeJob{p->last_w, base + w.wlast_t, CP_D_E, 512, 64, 0};
    hipLaunchKernelGGL((transpose_w_batch_kernel<T>), dim3(128, CP_N_FC + 1), dim3(256), 0, st, tb);
    CKL("transpose_w_batch_kernel");
    return 0;
}
static int launch_weight_transposes_fp8(const cp_params* p, unsigned char* base, const WS& w, hipStream_t st) {
    ProfScope ps(CP_K_PREP, st);
    const Fp8State* fs = (const Fp8State*)(base + w.f8state);
    Transpose8Batch tb{};
    for (int i = 0; i < CP_N_FC; ++i)
        tb.job[i] = Transpose8Job{p->fc_w[i], base + w.wfc8t[i], base + w.wsc8t[i], fcK(i), i == 0 ? 1 : 0, F8_T_GRAD + (i + 2)};
    hipLaunchKernelGGL(transpose_w8_batch_kernel, dim3(12, CP_N_FC, 4), dim3(256), 0, st, tb, fs);
    hipLaunchKernelGGL((transpose_w_kernel<bf16_t>), dim3(64), dim3(256), 0, st, p->last_w, (bf16_t*)(base + w.wlast_t), CP_D_E, 512, 64, 0);
    CKL("transpose kernels (fp8)");
    return 0;
}

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

extern "C" int cp_gather_oob_count(uint32_t* count_out, int32_t reset, void* stream) {
    if (!count_out) return fail(CP_ERR_ARG, "cp_gather_oob_count args");
    unsigned int* ctr = nullptr;
    CK(hipGetSymbolAddress((void**)&ctr, HIP_SYMBOL(g_gather_oob)));
    CK(hipMemcpyAsync(count_out, ctr, sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (reset) CK(hipMemsetAsync(ctr, 0, sizeof(uint32_t), (hipStream_t)stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// encoder forward
// ---------------------------------------------------------------------------------------
// Workgroup caps of the streaming passes around a dropout (bn_dropout_apply[8], bn_relu_bwd[8]).  Round 4, third part: 512 = two
// workgroups per CU.  With 4,096 / 2,048 a thread saw five / ten rows -- one batch of four loads in flight and a tail -- behind a
// prologue of 32 statistics loads; at 512 it walks 41 rows in batches of four.  Same box, traced steps, caps 256 / 384 / 512 / 768 /
// 1024 / 1536 / (4096 | 2048): bn_dropout_apply8 45 / 46 / 38-39 / 38 / 40 / 40 / 56-60 us, bn_relu_bwd8 53 / 46 / 43 / 44 / 49 / 57 / 54-57,
// bn_dropout_apply (bf16) 76 / 64 / 57-58 / 58-59 / 60 / 59 / 60, bn_relu_bwd 98 / 85 / 87 / 86-88 / 95 / 88 / 88-89 (the 16-bit passes
// were at the copy rate already).  The 8-bit step: 2,424-2,467 -> 2,315-2,354 us.
#define CAP_BDA16 512
#define CAP_BDA8 512
#define CAP_BRB16 512
#define CAP_BRB8 512
static inline int grid_rows(int64_t rows, int rows_per_block, int cap) {
    int64_t g = (rows + rows_per_block - 1) / rows_per_block;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

// fc-layer NT GEMM dispatch: bf16 runs the 256x256 LDS-DMA kernel (one 8-wave block per CU), f32
// (parity path) the 128x128 register-staged one.  fc_bm<T>() = rows per tile = rows per BN-partial row.
// (A 128x256-tile variant with two 4-wave blocks per CU was measured and dropped: 201 vs 148 us per
//  512x512 layer at 167,936 rows -- its 1.0 GB of L2->LDS fills per launch, against 0.67 GB, cost more
//  than overlapping one block's epilogue with the other's MFMAs gained)
template <typename T> static inline int fc_bm() { return sizeof(T) == 2 ? 256 : 128; }
// bf16 launches without saved-activation statistics (every forward launch, and the data gradients whose
// BN-backward sums come from the weight gradient) run the persistent kernel (gemm_nt256p.cuh).
// *stat_rows = number of partial rows of column sums the launch wrote.
template <typename T, int EPI>
static inline hipError_t launch_fc_gemm(const GemmNTArgs& a, hipStream_t st, int* stat_rows = nullptr, bool dyn_schedule = false) {
    if (stat_rows) *stat_rows = (int)((a.M + fc_bm<T>() - 1) / fc_bm<T>());
    if constexpr (sizeof(T) == 2) {
        // a process that has the GPU to itself (static schedule): the weight-stationary kernels (gemm_ws.cuh) -- K = 512 forward,
        // fc1 (K = 768) on its narrow form (32 features per wave), data gradients with BatchNorm + ReLU backward or (behind a dropout) the mask + sums
        const bool dyn = dyn_schedule, ws_ok = !dyn;
        if (EPI == EPI_FWD && a.K == WS_K && a.lda == WS_K && a.relu && ws_ok) return launch_gemm_ws(a, st, stat_rows);
        if (EPI == EPI_FWD && a.K == WSK_K && a.lda == WSK_K && a.F == 512 && a.relu && ws_ok) return launch_gemm_ws16n(a, st, stat_rows);
        if (EPI == EPI_FWD || (a.R == nullptr && a.dp_thresh == 0)) return launch_gemm_nt256p<EPI>(a, st, stat_rows, dyn);
        if (EPI == EPI_DGRAD && a.R != nullptr && a.K == WS_K && a.lda == WS_K && ws_ok) return launch_gemm_wsd_bn(a, st, stat_rows);
        // the persistent kernel's R epilogues (dynamic schedule, or K != 512): BN + ReLU backward of the layer below (coef), or
        // dropout + BN-backward sums
        if constexpr (EPI == EPI_DGRAD)
            return a.coef ? launch_gemm_nt256p<EPI_DGRAD_BN>(a, st, stat_rows, dyn) : launch_gemm_nt256p<EPI_DGRAD_ST>(a, st, stat_rows, dyn);
        return hipErrorInvalidValue;
    } else {
        return launch_gemm_nt<T, 128, 128, ALOAD_PLAIN, EPI>(a, st);
    }
}

// persistent conv strip kernels: blocks per CU allowed by their registers (bf16: 2) and LDS footprint (f32 100 KB: 1)
template <typename T>
static inline int conv_grid(int64_t n_windows) {
    const int64_t strips = (n_windows + CONV_WPB - 1) / CONV_WPB;
    const int64_t cap = sizeof(T) == 2 ? 512 : 256;
    return (int)(strips < cap ? strips : cap);
}

// fold many partial rows into REDUCE_SLICES rows (parallel) before a single-block finalize
struct PreReduce {
    const float* partials;
    float* scratch;
    hipStream_t st;
    // direct_rows: how many rows the consumer walks without help (the 16-lane finalize kernels: FIN_DIRECT_ROWS; kernels
    // that walk rows with one thread per column: 2 * REDUCE_SLICES)
    const float* operator()(int& nrows, int W, int direct_rows = FIN_DIRECT_ROWS) const {
        if (nrows <= direct_rows) return partials;
        hipLaunchKernelGGL(reduce_rows_kernel, dim3(W / 64, REDUCE_SLICES), dim3(256), 0, st, partials, nrows, W, scratch);
        nrows = REDUCE_SLICES;
        return scratch;
    }
};

// Synchronised BatchNorm: fold `nrows` partial rows of `width` floats into ONE row (this rank's sums, kept in ws.sync_loc),
// copy it, and have the caller's hook sum the copy over the ranks in place (ws.sync_glob).  Returns the global row;
// *local = this rank's row.  Stream-ordered: the hook enqueues its collective behind `st` and makes `st` wait for it.
static int sync_row(const cp_config* c, const float* pp, int nrows, int width, unsigned char* base, const WS& w, hipStream_t st,
                    const float** glob, const float** local, const int* unscale_exp = nullptr) {
    float* loc = (float*)(base + w.sync_loc);
    float* glo = (float*)(base + w.sync_glob);
    if (width > 2 * 768) return fail(CP_ERR_ARG, "sync_row width");
    // (CP_FP8 forward: every rank keeps its own scale table, so the row goes into TRUE units before it meets the other ranks')
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(width)), dim3(FIN_THREADS), 0, st, pp, nrows, width, loc, unscale_exp, width / 2);
    CKL("colsum_finalize_kernel(sync)");
    CK(hipMemcpyAsync(glo, loc, (size_t)width * 4, hipMemcpyDeviceToDevice, st));
    if (int e = c->stats_allreduce(c->stats_user, glo, width, st)) return fail(e, "the statistics all-reduce hook failed");
    *glob = glo;
    if (local) *local = loc;
    return 0;
}

template <typename T>
static int encoder_forward_t(const cp_config* c, const cp_params* p, const cp_bn_buffers* bn, const float* x,
                             unsigned char* base, const WS& w, float* z, hipStream_t st) {
    using D = DT<T>;
    const int64_t N = c->n_windows, R12 = N * 12;
    const bool batch_stats = c->training || c->adabn;
    const bool have_running = bn && bn->running_mean[0] && bn->running_var[0];
    if (!batch_stats && !have_running) return fail(CP_ERR_ARG, "eval with stock BN needs running statistics");
    const int upd = (c->training && !c->adabn && have_running) ? 1 : 0;
    const bool drop = c->training && c->dp_emg > 0.f;
    float* partials = (float*)(base + w.partials);
    auto act = [&](int l) { return (T*)(base + w.act[l]); };
    auto stats = [&](int l) { return (float*)(base + w.stats[l]); };
    auto finalize = [&](int l, int nrows, double count) -> int {
        if (!batch_stats) return 0;                       // evaluation with running statistics: all nine tables were written up front
        ProfScope ps(CP_K_BN_FINALIZE, st);
        const int C = kLayerC[l];
        const PreReduce pre{partials, (float*)(base + w.partials2), st};
        const float* pp = batch_stats ? pre(nrows, 2 * C) : partials;
        if (batch_stats && c->stats_allreduce) {          // synchronised BatchNorm: statistics of the GLOBAL batch
            if (int e = sync_row(c, pp, nrows, 2 * C, base, w, st, &pp, nullptr)) return e;
            nrows = 1;
            count *= c->stats_world;
        }
        hipLaunchKernelGGL(bn_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, st, pp, nrows, count, p->bn_g[l], p->bn_b[l],
                           have_running ? bn->running_mean[l] : nullptr, have_running ? bn->running_var[l] : nullptr, upd,
                           batch_stats ? 0 : 1, c->bn_momentum, c->bn_eps, stats(l), C);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail((int)e, "bn_finalize_kernel");
    };

    {
        ProfScope ps(CP_K_PREP, st);
        hipLaunchKernelGGL((prep_conv2_kernel<T>), dim3(48), dim3(256), 0, st, p->conv2_w, (T*)(base + w.wc2_f), (T*)(base + w.wc2_d));
        CKL("prep_conv2_kernel");
        if (!batch_stats) {
            BnRunningAll ra{};
            for (int l = 0; l < CP_N_BN; ++l) {
                ra.gamma[l] = p->bn_g[l]; ra.beta[l] = p->bn_b[l]; ra.mean[l] = bn->running_mean[l]; ra.var[l] = bn->running_var[l];
                ra.stats[l] = stats(l); ra.C[l] = kLayerC[l];
            }
            ra.eps = c->bn_eps;
            hipLaunchKernelGGL(bn_running_stats_kernel, dim3(CP_N_BN), dim3(512), 0, st, ra);
            CKL("bn_running_stats_kernel");
            // ... so every BatchNorm fold of the pass (fc1..fc7 and the projection) can be made now, in one launch instead of eight between the GEMMs
            FoldBnBatch fb{};
            for (int i = 0; i < CP_N_FC; ++i) {
                const int Lp = 1 + i;
                fb.job[i] = FoldBnJob{p->fc_w[i], p->fc_b[i], stats(Lp) + 2 * kLayerC[Lp], stats(Lp) + 3 * kLayerC[Lp], base + w.wfc[i],
                                      (float*)(base + w.bfc[i]), 512, fcK(i), i == 0 ? 1 : 0, 512};
            }
            fb.job[CP_N_FC] = FoldBnJob{p->last_w, nullptr, stats(8) + 2 * 512, stats(8) + 3 * 512, base + w.wlast, (float*)(base + w.blast), CP_D_E, 512, 0, 32};
            hipLaunchKernelGGL((fold_linear_batch_kernel<T>), dim3(512, CP_N_FC + 1), dim3(256), 0, st, fb);
            CKL("fold_linear_batch_kernel");
        }
        if (drop) {
            // the weights of the layers behind a dropout (fc5..fc7, projection) carry no BatchNorm fold: plain copies, all in one launch
            FoldBatch fb{};
            for (int q = 0; q < 3; ++q)
                fb.job[q] = FoldJob{p->fc_w[4 + q], p->fc_b[4 + q], base + w.wfc[4 + q], (float*)(base + w.bfc[4 + q]), 512, 512, 512};
            fb.job[3] = FoldJob{p->last_w, nullptr, base + w.wlast, (float*)(base + w.blast), CP_D_E, 512, 32};
            hipLaunchKernelGGL((fold_copy_batch_kernel<T>), dim3(512, 4), dim3(256), 0, st, fb);
            CKL("fold_copy_batch_kernel");
        }
    }
    // conv1
    {
        constexpr int RPP = 256 / (64 / D::EPC);                      // windows per block and pass
        const int64_t need = (N + RPP - 1) / RPP, passes = (need + 2047) / 2048;          // (caps 1024 / 512 measured: 23.6 / 23.8 us against 20.6)
        const int g = (int)((need + passes - 1) / passes);            // every block makes the same number of passes
        if (batch_stats) {                               // (evaluation with running statistics needs nothing of conv1 but its recomputation)
            ProfScope ps(CP_K_CONV1_FWD, st);
            // statistics only: r1 is never stored, its consumers recompute it from x (conv_kernels.cuh)
            hipLaunchKernelGGL((conv1_stats_kernel<T>), dim3(g), dim3(256), 0, st, x, p->conv1_w, p->conv1_b, partials, R12);
            CKL("conv1_stats_kernel");
        }
        if (int e = finalize(0, g, (double)R12)) return e;
    }
    // conv2
    {
        ConvArgs ca{};
        ca.x = x; ca.w1 = p->conv1_w; ca.b1 = p->conv1_b; ca.stats1 = stats(0);
        ca.wc = base + w.wc2_f; ca.bias2 = p->conv2_b; ca.out = act(1); ca.partials = batch_stats ? partials : nullptr; ca.n_windows = N;
        const int g = conv_grid<T>(N);
        {
            ProfScope ps(CP_K_CONV2_FWD, st);
            hipLaunchKernelGGL((conv2_strip_kernel<T, 0>), dim3(g), dim3(256), 0, st, ca);
            CKL("conv2_strip_kernel<fwd>");
        }
        if (int e = finalize(1, g, (double)R12)) return e;
    }
    // fc1..fc7
    for (int i = 0; i < CP_N_FC; ++i) {
        const int L = 2 + i, Lp = L - 1, K = fcK(i);
        const T* A = act(Lp);
        const float *s = stats(Lp) + 2 * kLayerC[Lp], *t = stats(Lp) + 3 * kLayerC[Lp];
        if (drop && Lp >= 5) {
            T* u = (T*)(base + w.u[Lp - 5]);
            ProfScope ps(CP_K_DROPOUT, st);
            hipLaunchKernelGGL((bn_dropout_apply_kernel<T>), dim3(grid_rows(N, 256 / (512 / D::EPC), CAP_BDA16)), dim3(256), 0, st,
                               act(Lp), stats(Lp), u, N, 512, dp_thresh(c->dp_emg), dp_key(c, Lp), dp_inv_keep(c->dp_emg), dp_salt(c));
            CKL("bn_dropout_apply_kernel");
            A = u; s = nullptr; t = nullptr;
        }
        if (!(drop && Lp >= 5) && batch_stats) {          // (the layers behind a dropout were copied by fold_copy_batch_kernel above; running statistics: folded up front)
            ProfScope ps(CP_K_FOLD, st);
            hipLaunchKernelGGL((fold_linear_kernel<T>), dim3(512), dim3(256), 0, st, p->fc_w[i], p->fc_b[i], s, t,
                               (T*)(base + w.wfc[i]), (float*)(base + w.bfc[i]), 512, K, i == 0 ? 1 : 0);
            CKL("fold_linear_kernel");
        }
        GemmNTArgs a{};
        a.A = A; a.lda = K; a.M = N; a.K = K;
        a.W = base + w.wfc[i]; a.F = 512;
        a.C = act(L); a.ldc = 512; a.bias = (float*)(base + w.bfc[i]); a.relu = 1;
        // (evaluation with the running statistics: nobody reads the column sums -- the weight-stationary kernels then skip them; the
        //  other dispatch targets ignore the distinction and write rows nobody reads)
        a.partials = (batch_stats || sizeof(T) != 2 || dyn_tiles(c)) ? partials : nullptr;
        int nrows = 0;
        {
            // (profiler kinds name ONE kernel each: K = 512 bf16 launches under the static schedule run gemm_ws16_kernel)
            const bool ws = sizeof(T) == 2 && K == WS_K && !dyn_tiles(c);
            ProfScope ps(ws ? CP_K_FC_FWD_WS : CP_K_FC_FWD, st);
            CK((launch_fc_gemm<T, EPI_FWD>(a, st, &nrows, dyn_tiles(c))));
        }
        if (int e = finalize(L, nrows, (double)N)) return e;
    }
    // projection 512 -> 16 (weights padded to 32 rows)
    {
        const int Lp = 8;
        const T* A = act(Lp);
        const float *s = stats(Lp) + 2 * 512, *t = stats(Lp) + 3 * 512;
        // dropout(BN(fc7)) is NOT written out for the projection: its two consumers (this launch and the projection's weight
        // gradient) form it from the saved activation while staging their operand -- both are bound by reading those 172 MB, and
        // the pass that materialised it moved 344 MB.  (That pass, as fc4..fc6 keep it, was removed here; see git history.)
        if (!drop && batch_stats) {        // (with dropout: copied by fold_copy_batch_kernel at the start of the pass; running statistics: folded up front)
            ProfScope ps(CP_K_FOLD, st);
            hipLaunchKernelGGL((fold_linear_kernel<T>), dim3(32), dim3(256), 0, st, p->last_w, (const float*)nullptr, s, t,
                               (T*)(base + w.wlast), (float*)(base + w.blast), CP_D_E, 512, 0);
            CKL("fold_linear_kernel(last)");
        }
        GemmNTArgs a{};
        a.A = A; a.lda = 512; a.M = N; a.K = 512;
        a.W = base + w.wlast; a.F = 32;
        a.C = z; a.ldc = CP_D_E; a.f_valid = CP_D_E; a.bias = (float*)(base + w.blast);
        {
            ProfScope ps(CP_K_PROJ_FWD, st);
            if (drop) {
                a.a_scale = stats(Lp) + 2 * 512; a.a_shift = stats(Lp) + 3 * 512;
                a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, Lp); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c);
                CK((launch_gemm_nt<T, 128, 32, ALOAD_BNDROP, EPI_PLAIN_F32>(a, st)));
            } else {
                CK((launch_gemm_nt<T, 128, 32, ALOAD_PLAIN, EPI_PLAIN_F32>(a, st)));
            }
        }
    }
    return 0;
}


// ---------------------------------------------------------------------------------------
// encoder forward, CP_FP8 (csrc/fp8.cuh): conv stack on the bf16 kernels with conv2's output stored as e4m3, fc1..fc7 on the
// block-scaled MFMA with e4m3 activations and weights, projection on the bf16 kernel with its operand converted while staging
// ---------------------------------------------------------------------------------------
static int encoder_forward_fp8(const cp_config* c, const cp_params* p, const cp_bn_buffers* bn, const float* x,
                               unsigned char* base, const WS& w, float* z, hipStream_t st) {
    using T = bf16_t;
    using D = DT<T>;
    const int64_t N = c->n_windows, R12 = N * 12;
    const bool batch_stats = c->training || c->adabn;
    const bool have_running = bn && bn->running_mean[0] && bn->running_var[0];
    if (!batch_stats && !have_running) return fail(CP_ERR_ARG, "eval with stock BN needs running statistics");
    // (cp_config.tile_schedule is not consulted: the 8-bit kernels are weight-stationary, i.e. statically scheduled; a packed sweep
    //  that asks for the dynamic schedule gets it on its 16/32-bit configurations)
    const int upd = (c->training && !c->adabn && have_running) ? 1 : 0;
    const bool drop = c->training && c->dp_emg > 0.f;
    float* partials = (float*)(base + w.partials);
    Fp8State* fs = (Fp8State*)(base + w.f8state);
    auto stats = [&](int l) { return (float*)(base + w.stats[l]); };
    auto finalize = [&](int l, int nrows, double count, const int* unscale) -> int {
        if (!batch_stats) return 0;                       // (encoder_forward_t: one launch wrote all nine tables)
        ProfScope ps(CP_K_BN_FINALIZE, st);
        const int C = kLayerC[l];
        const PreReduce pre{partials, (float*)(base + w.partials2), st};
        const float* pp = batch_stats ? pre(nrows, 2 * C) : partials;
        if (batch_stats && c->stats_allreduce) {          // synchronised BatchNorm: the row crosses the ranks in true units
            if (int e = sync_row(c, pp, nrows, 2 * C, base, w, st, &pp, nullptr, unscale)) return e;
            nrows = 1;
            count *= c->stats_world;
            unscale = nullptr;
        }
        hipLaunchKernelGGL(bn_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, st, pp, nrows, count, p->bn_g[l], p->bn_b[l],
                           have_running ? bn->running_mean[l] : nullptr, have_running ? bn->running_var[l] : nullptr, upd,
                           batch_stats ? 0 : 1, c->bn_momentum, c->bn_eps, stats(l), C, unscale);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail((int)e, "bn_finalize_kernel");
    };
    {
        ProfScope ps(CP_K_PREP, st);
        hipLaunchKernelGGL(fp8_update_scales_kernel, dim3(1), dim3(64), 0, st, fs, N);
        hipLaunchKernelGGL((prep_conv2_kernel<T>), dim3(48), dim3(256), 0, st, p->conv2_w, (T*)(base + w.wc2_f), (T*)(base + w.wc2_d));
        if (!batch_stats) {
            BnRunningAll ra{};
            for (int l = 0; l < CP_N_BN; ++l) {
                ra.gamma[l] = p->bn_g[l]; ra.beta[l] = p->bn_b[l]; ra.mean[l] = bn->running_mean[l]; ra.var[l] = bn->running_var[l];
                ra.stats[l] = stats(l); ra.C[l] = kLayerC[l];
            }
            ra.eps = c->bn_eps;
            hipLaunchKernelGGL(bn_running_stats_kernel, dim3(CP_N_BN), dim3(512), 0, st, ra);
        }
        if (batch_stats && drop) {
            // the folds of the layers behind a dropout (fc5..fc7: their operand is the dropout OUTPUT, no BatchNorm affine to fold) need
            // nothing of this pass but the scale table: one launch here instead of three between the GEMMs
            Fold8Batch fb{};
            for (int i = 4; i < CP_N_FC; ++i)
                fb.job[i - 4] = Fold8Job{p->fc_w[i], p->fc_b[i], nullptr, nullptr, base + w.wfc8[i], base + w.wsc8[i],
                                         (float*)(base + w.bfc[i]), fcK(i), 0, F8_T_U + (i - 4), F8_T_ACT + 2 + i};
            hipLaunchKernelGGL(fold_linear8_batch_kernel, dim3(512, CP_N_FC - 4), dim3(256), 0, st, fb, (const Fp8State*)fs);
        }
        CKL("prep kernels (fp8)");
    }
    // conv1 (statistics only) and conv2 (output as e4m3)
    {
        constexpr int RPP = 256 / (64 / D::EPC);
        const int64_t need = (N + RPP - 1) / RPP, passes = (need + 2047) / 2048;          // (caps 1024 / 512 measured: 23.6 / 23.8 us against 20.6)
        const int g = (int)((need + passes - 1) / passes);
        if (batch_stats) {
            ProfScope ps(CP_K_CONV1_FWD, st);
            hipLaunchKernelGGL((conv1_stats_kernel<T>), dim3(g), dim3(256), 0, st, x, p->conv1_w, p->conv1_b, partials, R12);
            CKL("conv1_stats_kernel");
        }
        if (int e = finalize(0, g, (double)R12, nullptr)) return e;
    }
    {
        ConvArgs ca{};
        ca.x = x; ca.w1 = p->conv1_w; ca.b1 = p->conv1_b; ca.stats1 = stats(0);
        ca.wc = base + w.wc2_f; ca.bias2 = p->conv2_b; ca.out = nullptr; ca.partials = batch_stats ? partials : nullptr; ca.n_windows = N;
        ca.out8 = base + w.act8[1]; ca.out_exp = &fs->e[F8_T_ACT + 1]; ca.out_amax = &fs->amax[F8_T_ACT + 1];
        const int g = conv_grid<T>(N);
        {
            ProfScope ps(CP_K_CONV2_FWD, st);
            hipLaunchKernelGGL((conv2_strip_kernel<T, 0>), dim3(g), dim3(256), 0, st, ca);
            CKL("conv2_strip_kernel<fwd, e4m3>");
        }
        if (int e = finalize(1, g, (double)R12, nullptr)) return e;      // (its sums are of the bf16-rounded values in true units)
    }
    if (!batch_stats) {
        // evaluation with the running statistics (no dropout): statistics and scale table are final, so the seven folds are one launch
        ProfScope ps(CP_K_FOLD, st);
        Fold8Batch fb{};
        for (int i = 0; i < CP_N_FC; ++i) {
            const int Lp = 1 + i;
            fb.job[i] = Fold8Job{p->fc_w[i], p->fc_b[i], stats(Lp) + 2 * kLayerC[Lp], stats(Lp) + 3 * kLayerC[Lp], base + w.wfc8[i], base + w.wsc8[i],
                                 (float*)(base + w.bfc[i]), fcK(i), i == 0 ? 1 : 0, F8_T_ACT + Lp, F8_T_ACT + 2 + i};
        }
        hipLaunchKernelGGL(fold_linear8_batch_kernel, dim3(512, CP_N_FC), dim3(256), 0, st, fb, (const Fp8State*)fs);
        CKL("fold_linear8_batch_kernel");
    }
    // fc1..fc7
    for (int i = 0; i < CP_N_FC; ++i) {
        const int L = 2 + i, Lp = L - 1, K = fcK(i);
        const bool in_drop = drop && Lp >= 5;
        const uint8_t* A = base + w.act8[Lp];
        int t_in = F8_T_ACT + Lp;
        const float *s = stats(Lp) + 2 * kLayerC[Lp], *t = stats(Lp) + 3 * kLayerC[Lp];
        if (in_drop) {
            uint8_t* u = base + w.u8[Lp - 5];
            t_in = F8_T_U + (Lp - 5);
            ProfScope ps(CP_K_DROPOUT, st);
            hipLaunchKernelGGL(bn_dropout_apply8_kernel, dim3(grid_rows(N, 256 / (512 / 16), CAP_BDA8)), dim3(256), 0, st, A, stats(Lp), u, N, 512,
                               dp_thresh(c->dp_emg), dp_key(c, Lp), dp_inv_keep(c->dp_emg), dp_salt(c), fs, F8_T_ACT + Lp, t_in);
            CKL("bn_dropout_apply8_kernel");
            A = u; s = nullptr; t = nullptr;
        }
        if (batch_stats && !in_drop) {     // (running statistics: all seven folds were made in one launch before the loop; behind a dropout: in the prep launch)
            ProfScope ps(CP_K_FOLD, st);
            hipLaunchKernelGGL(fold_linear8_kernel, dim3(512), dim3(256), 0, st, p->fc_w[i], p->fc_b[i], s, t, base + w.wfc8[i], base + w.wsc8[i],
                               (float*)(base + w.bfc[i]), K, i == 0 ? 1 : 0, fs, t_in, F8_T_ACT + L);
            CKL("fold_linear8_kernel");
        }
        Ws8Args a{};
        a.A = A; a.W = base + w.wfc8[i]; a.wsc = base + w.wsc8[i]; a.bias = (float*)(base + w.bfc[i]);
        a.C = base + w.act8[L]; a.partials = batch_stats ? partials : nullptr; a.amax = &fs->amax[F8_T_ACT + L]; a.M = N; a.F = 512;     // (nullptr: no column sums)
        int nrows = 0;
        {
            ProfScope ps(K == 512 ? CP_K_FC_FWD_WS : CP_K_FC_FWD, st);
            if (K == 512) CK(launch_gemm_ws8<512>(a, st, &nrows));
            else CK(launch_gemm_ws8<768>(a, st, &nrows));
        }
        if (int e = finalize(L, nrows, (double)N, &fs->e[F8_T_ACT + L])) return e;
    }
    // projection 512 -> 16 on the bf16 kernel: its operand is read as e4m3 and converted (and, with dropout, turned into
    // dropout(BN(fc7))) while staging
    {
        const int Lp = 8;
        const float *s = stats(Lp) + 2 * 512, *t = stats(Lp) + 3 * 512;
        {
            ProfScope ps(CP_K_FOLD, st);
            if (drop) hipLaunchKernelGGL((fold_linear_kernel<T>), dim3(32), dim3(256), 0, st, p->last_w, (const float*)nullptr, (const float*)nullptr,
                                         (const float*)nullptr, (T*)(base + w.wlast), (float*)(base + w.blast), CP_D_E, 512, 0);
            else hipLaunchKernelGGL((fold_linear_kernel<T>), dim3(32), dim3(256), 0, st, p->last_w, (const float*)nullptr, s, t,
                                    (T*)(base + w.wlast), (float*)(base + w.blast), CP_D_E, 512, 0);
            CKL("fold_linear_kernel(last)");
        }
        GemmNTArgs a{};
        a.A = base + w.act8[Lp]; a.lda = 512; a.M = N; a.K = 512;
        a.W = base + w.wlast; a.F = 32;
        a.C = z; a.ldc = CP_D_E; a.f_valid = CP_D_E; a.bias = (float*)(base + w.blast);
        a.a_exp = &fs->e[F8_T_ACT + Lp];
        ProfScope ps(CP_K_PROJ_FWD, st);
        if (drop) {
            a.a_scale = s; a.a_shift = t;
            a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, Lp); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c);
            CK((launch_gemm_nt<T, 128, 32, ALOAD_BNDROP_F8, EPI_PLAIN_F32>(a, st)));
        } else {
            CK((launch_gemm_nt<T, 128, 32, ALOAD_F8, EPI_PLAIN_F32>(a, st)));
        }
    }
    return 0;
}


// ---------------------------------------------------------------------------------------
// small batches (csrc/small.cuh): N <= 64 groups, batch statistics, f32 or bf16
// ---------------------------------------------------------------------------------------
static bool use_small(const cp_config* c) {
    return c->n_windows <= SM_MAX_WINDOWS && (c->training || c->adabn) && c->dtype != CP_FP8 && !c->stats_allreduce && !c->grad_tap &&
           !opt(c, CP_OPT_NO_SMALL);
}

template <typename T>
static int encoder_forward_small_t(const cp_config* c, const cp_params* p, const cp_bn_buffers* bn, const float* x,
                                   unsigned char* base, const WS& w, float* z, hipStream_t st) {
    using D = DT<T>;
    const int64_t N = c->n_windows, R12 = N * 12;
    const bool have_running = bn && bn->running_mean[0] && bn->running_var[0];
    const int upd = (c->training && !c->adabn && have_running) ? 1 : 0;
    const bool drop = c->training && c->dp_emg > 0.f;
    float* partials = (float*)(base + w.partials);
    auto act = [&](int l) { return (T*)(base + w.act[l]); };
    auto stats = [&](int l) { return (float*)(base + w.stats[l]); };
    const int tiles_m = (int)((N + SM_BM - 1) / SM_BM);
    const bool ks = sm_ksplit<T>(N);                   // few row tiles: 64-feature tiles with the contraction split over wave pairs
    {
        ProfScope ps(CP_K_PREP, st);
        SmPrepBatch cb{};
        for (int i = 0; i < CP_N_FC; ++i) cb.job[i] = SmCopyJob{p->fc_w[i], base + w.wfc[i], 512, fcK(i), 512, i == 0 ? 1 : 0};
        cb.job[CP_N_FC] = SmCopyJob{p->last_w, base + w.wlast, CP_D_E, 512, 32, 0};
        cb.njobs = CP_N_FC + 1; cb.zero = (long long*)(base + w.sm_acc); cb.nzero = 18 * 2 * 768;
        for (int i = 0; i < CP_N_FC; ++i) cb.tr[i] = TransposeJob{p->fc_w[i], base + w.wfc_t[i], 512, fcK(i), 512, i == 0 ? 1 : 0};
        cb.tr[CP_N_FC] = TransposeJob{p->last_w, base + w.wlast_t, CP_D_E, 512, 64, 0};
        cb.ntrans = CP_N_FC + 1;
        cb.conv2_w = p->conv2_w; cb.wc2_f = base + w.wc2_f; cb.wc2_d = base + w.wc2_d;
        hipLaunchKernelGGL((sm_prep_kernel<T>), dim3(SM_PREP_GX, cb.njobs + 1 + cb.ntrans + 1), dim3(256), 0, st, cb);
        CKL("prep kernels (small)");
    }
    // conv1 statistics and conv2: fixed-point totals like the fc stack's -- conv2's kernel finalises BatchNorm1 in its prologue, fc1's
    // launch finalises BatchNorm2 (no finalize launches)
    long long* accs = (long long*)(base + w.sm_acc);
    auto acc_of = [&](int l) { return accs + (size_t)l * 2 * 768; };
    auto bn_of = [&](int l) {
        SmBN b{};
        b.acc = acc_of(l); b.C = kLayerC[l]; b.count = l < 2 ? (double)R12 : (double)N;
        b.gamma = p->bn_g[l]; b.beta = p->bn_b[l]; b.stats = stats(l);
        b.running_mean = have_running ? bn->running_mean[l] : nullptr; b.running_var = have_running ? bn->running_var[l] : nullptr;
        b.update_running = upd; b.momentum = c->bn_momentum; b.eps = c->bn_eps;
        return b;
    };
    {
        constexpr int RPP = 256 / (64 / D::EPC);
        const int64_t need = (N + RPP - 1) / RPP, passes = (need + 2047) / 2048;          // (caps 1024 / 512 measured: 23.6 / 23.8 us against 20.6)
        const int g = (int)((need + passes - 1) / passes);
        ProfScope ps(CP_K_CONV1_FWD, st);
        hipLaunchKernelGGL((conv1_stats_kernel<T>), dim3(g), dim3(256), 0, st, x, p->conv1_w, p->conv1_b, partials, R12, acc_of(0));
        CKL("conv1 (small)");
    }
    {
        ConvArgs ca{};
        ca.x = x; ca.w1 = p->conv1_w; ca.b1 = p->conv1_b; ca.stats1 = nullptr; ca.bn1 = bn_of(0); ca.acc_out = acc_of(1);
        ca.wc = base + w.wc2_f; ca.bias2 = p->conv2_b; ca.out = act(1); ca.partials = partials; ca.n_windows = N;
        const int g2 = conv_grid<T>(N);
        ProfScope ps(CP_K_CONV2_FWD, st);
        hipLaunchKernelGGL((conv2_strip_kernel<T, 0>), dim3(g2), dim3(256), 0, st, ca);
        CKL("conv2 (small)");
    }
    // fc1..fc7 and the projection: each launch turns its input's two fixed-point totals per column into scale / shift itself
    for (int i = 0; i < CP_N_FC; ++i) {
        const int L = 2 + i, Lp = L - 1, K = fcK(i);
        SmFwdArgs a{};
        a.A = act(Lp); a.W = base + w.wfc[i]; a.bias = p->fc_b[i]; a.C = act(L); a.out_acc = acc_of(L);
        a.bn_in = bn_of(Lp); a.smod = kLayerC[Lp]; a.N = N; a.K = K;
        if (drop && Lp >= 5) { a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, Lp); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c); }
        ProfScope ps(K == 512 ? CP_K_FC_FWD_WS : CP_K_FC_FWD, st);
        if (ks) hipLaunchKernelGGL((sm_fc_fwd_kernel<T, 0, true>), dim3(tiles_m * (512 / SmTile<true>::BN)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sm_fc_fwd_kernel<T, 0>), dim3(tiles_m * (512 / SM_BN)), dim3(256), 0, st, a);
        CKL("sm_fc_fwd_kernel");
    }
    {
        SmFwdArgs a{};
        a.A = act(8); a.W = base + w.wlast; a.C = z; a.bn_in = bn_of(8); a.smod = 512; a.N = N; a.K = 512;
        if (drop) { a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, 8); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c); }
        ProfScope ps(CP_K_PROJ_FWD, st);
        hipLaunchKernelGGL((sm_fc_fwd_kernel<T, 1>), dim3(tiles_m), dim3(256), 0, st, a);
        CKL("sm_fc_fwd_kernel<proj>");
    }
    return 0;
}

template <typename T> static int conv_backward_tail(const cp_config*, const cp_params*, const float*, unsigned char*, const WS&, cp_params*, hipStream_t,
                                                    hipEvent_t, T*, T*, bool, int, const Aux* aux = nullptr, int gcol_rows = 0,
                                                    const Fp8State* g8 = nullptr, bool small = false);

template <typename T>
static int encoder_backward_small_t(const cp_config* c, const cp_params* p, const float* x, unsigned char* base, const WS& w,
                                    cp_params* g, hipStream_t st, hipEvent_t fc_grads_ready) {
    const int64_t N = c->n_windows;
    const bool drop = c->training && c->dp_emg > 0.f;
    float* partials = (float*)(base + w.partials);
    auto act = [&](int l) { return (T*)(base + w.act[l]); };
    auto stats = [&](int l) { return (float*)(base + w.stats[l]); };
    const int tiles_m = (int)((N + SM_BM - 1) / SM_BM);
    const bool ks = sm_ksplit<T>(N);
    const int bn_tile = ks ? SmTile<true>::BN : SM_BN;
    // (the transposed weights the data gradients read were made by the forward pass's preparation launch: sm_prep_kernel)
    long long* accs = (long long*)(base + w.sm_acc);
    auto gacc_of = [&](int l) { return accs + (size_t)(9 + l) * 2 * 768; };        // totals of (g, g r_l) for layer l's BatchNorm backward
    T* gb[2] = {(T*)(base + w.gbuf[0]), (T*)(base + w.gbuf[1])};
    // weight gradients: whole-batch sums per tile up to 256 rows; more rows are split over workgroups (at most 8 splits, each into
    // its own slab of all the step's weight gradients) and summed by ONE launch at the end
    // (one split at 8 groups = 328 rows, without slabs and their reduction launch, measured SLOWER: 13.3 us per launch instead of
    //  10.3 -- the weight-gradient blocks walk all the rows, six steps of a latency-bound loop -- 21 us lost for 12.7 us gained)
    int splits = (int)((N + 255) / 256);
    if (splits > 8) splits = 8;
    int64_t rps = ((N + splits - 1) / splits + 63) / 64 * 64;
    splits = (int)((N + rps - 1) / rps);
    const int64_t kSlabStride = (int64_t)1 << 21;
    float* slabs = (float*)(base + w.slabs);
    size_t slab_off = 0;
    SmReduceBatch rb{};
    rb.splits = splits; rb.slab_stride = kSlabStride;
    auto grad_dst = [&](float* real, int numel) -> float* {          // where a role-1 block writes split 0 of this tensor
        if (splits == 1) return real;
        float* sl = slabs + slab_off;
        rb.job[rb.njobs++] = SmReduceJob{sl, real, numel};
        slab_off += (size_t)numel;
        return sl;
    };
    int cur = 0;
    {
        SmBwdArgs a{};
        a.Gin = base + w.dz; a.Wt = base + w.wlast_t; a.Rp = act(8); a.stats_p = stats(8); a.Gout = gb[cur]; a.out_acc = gacc_of(8);
        a.dW = grad_dst(g->last_w, CP_D_E * 512); a.db = nullptr; a.slab_stride = kSlabStride; a.rows_per_split = rps; a.splits = splits;
        a.p_valid = CP_D_E; a.N = N; a.K = 512; a.smod = 512; a.wmode = 0; a.n_dgrad = tiles_m * (512 / bn_tile);
        if (drop) { a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, 8); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c); }
        ProfScope ps(CP_K_PROJ_BWD, st);
        if (ks) hipLaunchKernelGGL((sm_fc_bwd_kernel<T, true, true>), dim3(a.n_dgrad + 8 * splits), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sm_fc_bwd_kernel<T, true>), dim3(a.n_dgrad + 8 * splits), dim3(256), 0, st, a);
        CKL("sm_fc_bwd_kernel<proj>");
    }
    for (int L = 8; L >= 2; --L) {
        const int i = L - 2, Lp = L - 1, K = fcK(i);
        SmBwdArgs a{};
        a.Gin = gb[cur]; a.R = act(L); a.gsum = gacc_of(L); a.stats = stats(L);
        a.dgamma = g->bn_g[L]; a.dbeta = g->bn_b[L]; a.Wt = base + w.wfc_t[i]; a.Rp = act(Lp); a.stats_p = stats(Lp);
        a.Gout = gb[cur ^ 1];
        if (Lp == 1) a.out_partials = partials;          // fc1: partial rows [tiles_m][2][768] for the conv tail's finalize launch
        else a.out_acc = gacc_of(Lp);
        a.dW = grad_dst(g->fc_w[i], 512 * K); a.db = grad_dst(g->fc_b[i], 512);
        a.slab_stride = kSlabStride; a.rows_per_split = rps; a.splits = splits; a.p_valid = 512;
        a.N = N; a.K = K; a.smod = kLayerC[Lp]; a.wmode = i == 0 ? 1 : 0; a.n_dgrad = tiles_m * (K / bn_tile);
        if (drop && Lp >= 5) { a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, Lp); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c); }
        ProfScope ps(CP_K_FC_DGRAD, st);
        if (ks) hipLaunchKernelGGL((sm_fc_bwd_kernel<T, false, true>), dim3(a.n_dgrad + 8 * (K / 64) * splits), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sm_fc_bwd_kernel<T, false>), dim3(a.n_dgrad + 8 * (K / 64) * splits), dim3(256), 0, st, a);
        CKL("sm_fc_bwd_kernel");
        cur ^= 1;
    }
    if (splits > 1) {
        ProfScope ps(CP_K_REDUCE_SLABS, st);
        hipLaunchKernelGGL(sm_reduce_grads_kernel, dim3(96, rb.njobs), dim3(256), 0, st, rb);
        CKL("sm_reduce_grads_kernel");
    }
    // `partials` now holds fc1's partial sums [tiles_m][2][768]: the conv tail finalises conv2's BatchNorm backward from them
    return conv_backward_tail<T>(c, p, x, base, w, g, st, fc_grads_ready, gb[cur], gb[cur ^ 1], false, tiles_m, nullptr, 0, nullptr, true);
}

// The kernel path of a forward pass (cp_forward_record.path): the backward pass must take the same one -- the small-batch form and the
// large-batch form leave different things in the workspace.
enum { PATH_LARGE = 0, PATH_SMALL = 1, PATH_FP8 = 2 };
static int forward_path(const cp_config* cfg) { return cfg->dtype == CP_FP8 ? PATH_FP8 : use_small(cfg) ? PATH_SMALL : PATH_LARGE; }

extern "C" int cp_encoder_forward(const cp_config* cfg, const cp_params* p, const cp_bn_buffers* bn, const float* x,
                                  void* ws, size_t ws_bytes, float* z_out, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (!p || !x || !z_out) return fail(CP_ERR_ARG, "cp_encoder_forward args");
    if (((uintptr_t)x & 15) != 0) return fail(CP_ERR_ARG, "x must be 16-byte aligned");
    // second stream (cp_config.aux_stream): the transposed weights of the backward pass are made beside the forward pass -- bf16 from its
    // start, CP_FP8 behind it (their scale bytes need this step's gradient exponents, set by the forward's first launch)
    const int path = forward_path(cfg);
    const bool drop = cfg->training && cfg->dp_emg > 0.f;
    const Aux aux = make_aux(cfg, (hipStream_t)stream, drop && path != PATH_SMALL && cfg->dtype != CP_F32 && !dyn_tiles(cfg) &&
                                                           !opt(cfg, CP_OPT_UNPAIRED_WGRAD) && !opt(cfg, CP_OPT_UNFUSED_BN_BWD) && !opt(cfg, CP_OPT_FP8_BRIDGE));
    if (cp_forward_record* r = cfg->record)
        *r = cp_forward_record{cfg->n_windows, path, 0, aux.on ? 1 : 0, 0, aux.on ? (void*)aux.join_ev : nullptr};
    if (cfg->dtype == CP_FP8) {
        if (int e = encoder_forward_fp8(cfg, p, bn, x, (unsigned char*)ws, w, z_out, (hipStream_t)stream)) return e;
        if (aux.on) {
            if (int e = aux.fork()) return e;
            if (int e = launch_weight_transposes_fp8(p, (unsigned char*)ws, w, aux.side)) return e;
            CK(hipEventRecord(aux.join_ev, aux.side));          // (waited for by cp_encoder_backward)
        }
        return 0;
    }
    if (aux.on) {
        if (int e = aux.fork()) return e;
        if (int e = launch_weight_transposes<bf16_t>(p, (unsigned char*)ws, w, aux.side)) return e;
        CK(hipEventRecord(aux.join_ev, aux.side));
    }
    if (use_small(cfg)) {
        if (cfg->dtype == CP_BF16) return encoder_forward_small_t<bf16_t>(cfg, p, bn, x, (unsigned char*)ws, w, z_out, (hipStream_t)stream);
        return encoder_forward_small_t<float>(cfg, p, bn, x, (unsigned char*)ws, w, z_out, (hipStream_t)stream);
    }
    if (cfg->dtype == CP_BF16)
        return encoder_forward_t<bf16_t>(cfg, p, bn, x, (unsigned char*)ws, w, z_out, (hipStream_t)stream);
    return encoder_forward_t<float>(cfg, p, bn, x, (unsigned char*)ws, w, z_out, (hipStream_t)stream);
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
                     float* logits, cp_params* grads, const float* gneg, void* stream);

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

static int head_impl(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels, int64_t n_groups,
                     int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, float* loss_correct, int32_t* pred,
                     float* logits, cp_params* grads, const float* gneg, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (!p || !z || !labels || !loss_correct || !pred || V <= 0 || n_groups * CP_TASKS != cfg->n_windows)
        return fail(CP_ERR_ARG, "cp_head args");
    if (want_grad && (!grads || !grads->easy_w || !grads->easy_b)) return fail(CP_ERR_ARG, "cp_head grads");
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
    const int blocks = grid_rows(n_groups, HEAD_WAVES * (n_groups >= 2048 ? 2 : 1), kHeadBlocksMax);   // (>= 2048 groups: two per wave, half the prologues)
    // CP_FP8 (BASELINE config 4): the logits on the block-scaled 8-bit MFMA; "fp8_head_f32" keeps the f32 products (tests)
    const bool f8l = cfg->dtype == CP_FP8 && !opt(cfg, CP_OPT_FP8_HEAD_F32);
    if (cfg->dtype != CP_F32) {
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
                       want_grad, loss_correct, want_grad ? grads->easy_w : nullptr, want_grad ? grads->easy_b : nullptr);
    CKL("head_finalize_kernel");
    return 0;
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
// encoder backward
// ---------------------------------------------------------------------------------------
// test aid (cp_config.grad_tap): device buffer of 9 slots x n_windows x 768 elements of the compute dtype that receives a
// copy of every intermediate gradient of the backward pass, so that each backward kernel can be checked on its own
// inputs at full batch size (tests/test_gpu_fullsize.py).  nullptr (the default) = no copies.
static int tap_gradient(const cp_config* c, int slot, const void* src, int64_t n_windows, int width, size_t es, hipStream_t st) {
    if (!c->grad_tap) return 0;
    const size_t slot_bytes = (size_t)n_windows * 768 * es, bytes = (size_t)n_windows * width * es;
    if ((size_t)(slot + 1) * slot_bytes > c->grad_tap_bytes) return fail(CP_ERR_ARG, "gradient tap buffer too small");
    CK(hipMemcpyAsync((unsigned char*)c->grad_tap + slot * slot_bytes, src, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

static inline void split_rows(int64_t M, int target_splits, int* splits, int64_t* rows_per_split);

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
    if (cfg->dtype != CP_F32) return glove_forward_t<bf16_t>(cfg, gp, glove, rows, (unsigned char*)gws, w, zg, (hipStream_t)stream);
    return glove_forward_t<float>(cfg, gp, glove, rows, (unsigned char*)gws, w, zg, (hipStream_t)stream);
}

extern "C" int cp_head_glove(const cp_config* cfg, const float* z, const float* zg, const int64_t* labels, int64_t n_groups,
                             int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, void* gws, size_t gws_bytes,
                             float* loss_correct, int32_t* pred, float* logits, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (!z || !zg || !labels || !loss_correct || !pred || V <= 0 || n_groups * CP_TASKS != cfg->n_windows || n_groups % V != 0)
        return fail(CP_ERR_ARG, "cp_head_glove args");
    if (want_grad && V != 1) return fail(CP_ERR_ARG, "cp_head_glove: gradients need V == 1 (training batches)");
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
    const int blocks = grid_rows(n_groups, HEAD_WAVES * (n_groups >= 2048 ? 2 : 1), kHeadBlocksMax);   // (>= 2048 groups: two per wave, half the prologues)
    if (cfg->dtype != CP_F32)
        hipLaunchKernelGGL((head_kernel<bf16_t, true>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((head_kernel<float, true>), dim3(blocks), dim3(256), 0, st, a);
    CKL("head_kernel<glove>");
    int nr = blocks;
    const PreReduce pre{a.partials, (float*)(base + w.partials2), st};
    const float* pp = pre(nr, HEAD_PART, 2 * REDUCE_SLICES);
    hipLaunchKernelGGL(head_finalize_kernel, dim3(1), dim3(256), 0, st, pp, nr, n_groups, (const float*)nullptr, (const float*)nullptr,
                       0, loss_correct, (float*)nullptr, (float*)nullptr);
    CKL("head_finalize_kernel");
    return 0;
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

static inline void split_rows(int64_t M, int target_splits, int* splits, int64_t* rows_per_split) {
    int64_t rps = (M + target_splits - 1) / target_splits;
    rps = ((rps + 31) / 32) * 32;
    if (rps < 32) rps = 32;
    *rows_per_split = rps;
    *splits = (int)((M + rps - 1) / rps);
}

// conv stack of the backward pass (shared by the 16/32-bit and the 8-bit fc paths): cur = dL/d(BN2 output), or dL/d(conv2
// pre-activation) when bn_done, as [N][768] == [(N*12)][64] T; nxt = scratch of the same size
template <typename T>
static int conv_backward_tail(const cp_config* c, const cp_params* p, const float* x, unsigned char* base, const WS& w,
                              cp_params* g, hipStream_t st, hipEvent_t fc_grads_ready, T* cur, T* nxt, bool bn_done, int stat_rows, const Aux* aux,
                              int gcol_rows, const Fp8State* g8, bool small) {
    // small (the small-batch step, csrc/small.cuh: !bn_done, `partials` = fc1's partial rows [stat_rows][2][768]): four launches -- every
    // BatchNorm-backward finalisation happens in the consumer's prologue, BatchNorm2 + ReLU backward while conv2's weight gradient stages
    // g8 (CP_FP8): `cur` holds e5m2 bytes with the scale of tensor F8_T_GRAD + 1 (fc1's data-gradient launch wrote them), expanded into
    // the kernels' bf16 images while they are staged; the bias-gradient rows (gcol_rows) are in true units
    using D = DT<T>;
    const int64_t N = c->n_windows, R12 = N * 12;
    float* partials = (float*)(base + w.partials);
    // (round 4: conv2's weight gradient is on the critical path again -- BatchNorm1's backward sums follow from it -- so nothing of
    //  the conv stack floats on the second stream)
    float* slabs = (float*)(base + w.slabs);
    float* coef = (float*)(base + w.coef);
    float* rows2 = (float*)(base + w.partials2);
    auto act = [&](int l) { return (T*)(base + w.act[l]); };
    auto stats = [&](int l) { return (float*)(base + w.stats[l]); };
    const PreReduce pre{partials, rows2, st};
    auto bwd_finalize = [&](const float* pp, int nr, double count, int l, int C, int nfold, const char* what) -> int {
        const float* local = nullptr;
        if (c->stats_allreduce) {
            if (int e = sync_row(c, pp, nr, 2 * C * nfold, base, w, st, &pp, &local)) return e;
            nr = 1;
            count *= c->stats_world;
        }
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, st, pp, nr, count, stats(l), coef, g->bn_g[l],
                           g->bn_b[l], C, nfold, local);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail((int)e, what);
    };
    // every gradient but the conv stack's is final here (cp_encoder_backward_ev): a data-parallel caller starts summing
    // them across ranks while the conv backward below still runs
    if (fc_grads_ready) {
        if (aux) { if (int e = aux->join()) return e; }          // (the fc weight gradients that ran on the second stream included)
        CK(hipEventRecord(fc_grads_ready, st));
    }
    // ---- conv2: cur = dL/d(BN2 output) as [N][768] == [(N*12)][64] -------------------------
    if (small) {
        if (bn_done || g8 || c->stats_allreduce) return fail(CP_ERR_ARG, "conv_backward_tail: small-batch form");
        ConvArgs ca{};
        ca.x = x; ca.w1 = p->conv1_w; ca.b1 = p->conv1_b; ca.stats1 = nullptr; ca.gin = cur; ca.n_windows = N;
        float* gcols3 = (float*)(base + w.praw);
        const int64_t strips = (N + CONV_WG_WPB - 1) / CONV_WG_WPB;
        const int S = (int)(strips < 512 ? strips : 512);
        {
            ProfScope ps(CP_K_CONV2_WGRAD, st);
            ca.partials = slabs; ca.bn2_rows = partials; ca.bn2_nr = stat_rows; ca.r2 = act(1); ca.stats2 = stats(1);
            ca.dgamma2 = g->bn_g[1]; ca.dbeta2 = g->bn_b[1]; ca.gcols3 = gcols3;
            hipLaunchKernelGGL((conv2_wgrad_kernel<T, false, true>), dim3(S), dim3(256), 0, st, ca);
            CKL("conv2_wgrad_kernel<small>");
            const float* sl = slabs;
            int ns = S;
            if (S > 2 * REDUCE_SLICES) {
                float* folded = slabs + (size_t)S * 64 * 192;
                hipLaunchKernelGGL(reduce_rows_kernel, dim3(64 * 192 / 64, REDUCE_SLICES), dim3(256), 0, st, slabs, S, 64 * 192, folded);
                sl = folded;
                ns = REDUCE_SLICES;
            }
            hipLaunchKernelGGL((conv2_wgrad_finish_kernel<T>), dim3(CONV2_FINISH_ROWS), dim3(256), 0, st, sl, ns, (const float*)nullptr, S, p->conv2_w,
                               stats(0), g->conv2_w, rows2, (const float*)gcols3, g->conv2_b);
            CKL("conv2_wgrad_finish_kernel<small>");
        }
        if (int e = tap_gradient(c, 1, cur, N, 768, sizeof(T), st)) return e;         // dL/d(conv2 pre-activation): written back in place
        const int grid_d = conv_grid<T>(N);
        ca.wc = base + w.wc2_d;
        if (c->grad_tap) {
            ca.out = nxt; ca.partials = partials;
            hipLaunchKernelGGL((conv2_strip_kernel<T, 1>), dim3(grid_d), dim3(256), 0, st, ca);
            CKL("conv2_strip_kernel<dgrad> (gradient tap)");
            if (int e = tap_gradient(c, 0, nxt, N, 768, sizeof(T), st)) return e;
        }
        {
            ProfScope ps(CP_K_CONV2_DGRAD, st);
            ca.out = nullptr; ca.partials = partials; ca.stats1 = stats(0); ca.rows1 = rows2; ca.rows1_nr = CONV2_FINISH_ROWS;
            ca.dgamma1 = g->bn_g[0]; ca.dbeta1 = g->bn_b[0];
            hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T, false, true>), dim3(grid_d), dim3(256), 0, st, ca);
            CKL("conv2_dgrad_conv1_kernel<small>");
        }
        {
            ProfScope ps(CP_K_CONV1_BWD, st);
            int nr = grid_d;
            const float* pp = pre(nr, 4 * 64, 2 * REDUCE_SLICES);
            hipLaunchKernelGGL(conv1_bwd_finalize_kernel, dim3(1), dim3(256), 0, st, pp, nr, g->conv1_w, g->conv1_b);
            CKL("conv1_bwd_finalize_kernel");
        }
        if (aux) { if (int e = aux->join()) return e; }
        return 0;
    }
    if (!bn_done) {
        ProfScope ps(CP_K_BN_BWD, st);
        int nr = stat_rows;          // 1: fc1's input (conv2's BN) never has dropout
        const float* pp = pre(nr, 2 * 768);
        if (int e = bwd_finalize(pp, nr, (double)R12, 1, 64, 12, "bn_bwd_finalize_kernel(conv2)")) return e;
        const int gb = grid_rows(R12, 256 / (64 / D::EPC), 2048);
        hipLaunchKernelGGL((bn_relu_bwd_kernel<T>), dim3(gb), dim3(256), 256 * D::EPC * 4, st, cur, act(1), coef, partials, R12, 64);
        nr = gb;
        pp = pre(nr, 64);
        hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(64)), dim3(FIN_THREADS), 0, st, pp, nr, 64, g->conv2_b);
        CKL("bn_relu_bwd_kernel(conv2)");
        gcol_rows = 0;
    }
    const int* gexp = g8 ? (const int*)&g8->e[F8_T_GRAD + 1] : nullptr;
    if (g8) {
        if (gcol_rows <= 0 || sizeof(T) != 2) return fail(CP_ERR_ARG, "conv_backward_tail: 8-bit gradient without its column sums");
        if (c->grad_tap) {
            const size_t slot_bytes = (size_t)N * 768 * 2;
            if (2 * slot_bytes > c->grad_tap_bytes) return fail(CP_ERR_ARG, "gradient tap buffer too small");
            hipLaunchKernelGGL(dequant5_bf16_kernel, dim3(1024), dim3(256), 0, st, (const uint8_t*)cur, (bf16_t*)((unsigned char*)c->grad_tap + slot_bytes),
                               N * 192, g8, F8_T_GRAD + 1);
            CKL("dequant5_bf16_kernel(conv2 gradient)");
        }
    } else if (int e = tap_gradient(c, 1, cur, N, 768, sizeof(T), st)) return e;         // dL/d(conv2 pre-activation), [w][c]
    // column sums of that gradient per (position, channel): `partials` still holds them as fc1's data-gradient launch wrote them
    // (gcol_rows rows of 768, its bias-gradient rows); a caller without such rows gets them from one pass over the tensor
    if (gcol_rows <= 0) {
        constexpr int cpr = 768 / D::EPC, rpp = 256 / cpr;
        int64_t gb = (N + rpp - 1) / rpp;
        if (gb > 256) gb = 256;
        ProfScope ps(CP_K_BN_BWD, st);
        hipLaunchKernelGGL((colsum_kernel<T>), dim3((int)gb), dim3(256), (size_t)rpp * 768 * 4, st, cur, partials, N, 768, 768);
        CKL("colsum_kernel(conv2 gradient)");
        gcol_rows = (int)gb;
    }
    ConvArgs ca{};
    ca.x = x; ca.w1 = p->conv1_w; ca.b1 = p->conv1_b; ca.stats1 = nullptr; ca.gin = cur; ca.gin_exp = gexp; ca.n_windows = N;
    {
        // the RAW product g^T r1 (the image holds conv1's rounded ReLU output): BatchNorm1's scale and shift are applied to the
        // 64 x 192 result, and the same product gives BatchNorm1's backward sums (conv2_wgrad_finish_kernel)
        ProfScope ps(CP_K_CONV2_WGRAD, st);
        const int64_t strips = (N + CONV_WG_WPB - 1) / CONV_WG_WPB;
        const int64_t cap = sizeof(T) == 2 ? 512 : 256;      // two blocks per CU (194 registers with the strip prefetch)
        const int S = (int)(strips < cap ? strips : cap);
        ca.partials = slabs;
        if constexpr (sizeof(T) == 2) {
            if (g8) hipLaunchKernelGGL((conv2_wgrad_kernel<T, true>), dim3(S), dim3(256), 0, st, ca);
            else hipLaunchKernelGGL((conv2_wgrad_kernel<T>), dim3(S), dim3(256), 0, st, ca);
        } else {
            hipLaunchKernelGGL((conv2_wgrad_kernel<T>), dim3(S), dim3(256), 0, st, ca);
        }
        CKL("conv2_wgrad_kernel");
        // up to 512 slabs of 64x192: fold them into REDUCE_SLICES slabs in parallel first (scratch = the
        // unused tail of the slab buffer), then the finish kernel walks 32 instead of 512
        const float* sl = slabs;
        int ns = S;
        if (S > 2 * REDUCE_SLICES) {
            float* folded = slabs + (size_t)S * 64 * 192;
            hipLaunchKernelGGL(reduce_rows_kernel, dim3(64 * 192 / 64, REDUCE_SLICES), dim3(256), 0, st, slabs, S, 64 * 192, folded);
            sl = folded;
            ns = REDUCE_SLICES;
        }
        hipLaunchKernelGGL((conv2_wgrad_finish_kernel<T>), dim3(CONV2_FINISH_ROWS), dim3(256), 0, st, sl, ns, partials, gcol_rows, p->conv2_w, stats(0),
                           g->conv2_w, rows2);
        CKL("conv2_wgrad_finish_kernel");
    }
    {
        ProfScope ps(CP_K_BN_BWD, st);
        if (int e = bwd_finalize(rows2, CONV2_FINISH_ROWS, (double)R12, 0, 64, 1, "bn_bwd_finalize_kernel(conv1)")) return e;
    }
    const int grid_d = conv_grid<T>(N);
    ca.wc = base + w.wc2_d; ca.coef = coef;
    if (c->grad_tap) {
        // test aid: dL/d(BN1 output) is not a tensor of the step any more; the tap gets it from the stand-alone data-gradient kernel
        ca.out = nxt; ca.partials = partials;
        if (g8) ca.gin = (unsigned char*)c->grad_tap + (size_t)N * 768 * 2;          // (its bf16 expansion in tap slot 1)
        hipLaunchKernelGGL((conv2_strip_kernel<T, 1>), dim3(grid_d), dim3(256), 0, st, ca);
        ca.gin = cur;
        CKL("conv2_strip_kernel<dgrad> (gradient tap)");
        if (int e = tap_gradient(c, 0, nxt, N, 768, sizeof(T), st)) return e;         // dL/d(BN1 output), [w][c]
    }
    // ---- conv2's data gradient, BatchNorm1 + ReLU backward and conv1's gradients in one pass over cur ------------------
    {
        ProfScope ps(CP_K_CONV2_DGRAD, st);
        ca.out = nullptr; ca.partials = partials;
        if constexpr (sizeof(T) == 2) {
            if (g8) hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T, true>), dim3(grid_d), dim3(256), 0, st, ca);
            else hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T>), dim3(grid_d), dim3(256), 0, st, ca);
        } else {
            hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T>), dim3(grid_d), dim3(256), 0, st, ca);
        }
        CKL("conv2_dgrad_conv1_kernel");
    }
    {
        ProfScope ps(CP_K_CONV1_BWD, st);
        int nr = grid_d;
        const float* pp = pre(nr, 4 * 64, 2 * REDUCE_SLICES);
        hipLaunchKernelGGL(conv1_bwd_finalize_kernel, dim3(1), dim3(256), 0, st, pp, nr, g->conv1_w, g->conv1_b);
        CKL("conv1_bwd_finalize_kernel");
    }
    if (aux) { if (int e = aux->join()) return e; }      // everything the second stream was given is part of this call
    return 0;
}

template <typename T>
static int encoder_backward_t(const cp_config* c, const cp_params* p, const float* x, unsigned char* base, const WS& w,
                              cp_params* g, hipStream_t st, hipEvent_t fc_grads_ready, bool tposed = false) {
    using D = DT<T>;
    const int64_t N = c->n_windows, R12 = N * 12;
    const bool drop = c->training && c->dp_emg > 0.f;
    float* partials = (float*)(base + w.partials);
    float* slabs = (float*)(base + w.slabs);
    float* coef = (float*)(base + w.coef);
    auto act = [&](int l) { return (T*)(base + w.act[l]); };
    auto stats = [&](int l) { return (float*)(base + w.stats[l]); };
    const int tiles_n = (int)((N + fc_bm<T>() - 1) / fc_bm<T>());
    int gcol_rows = 0;           // partial rows [768] of fc1's data-gradient launch: column sums of dL/d(conv2 pre-activation)
    int stat_rows = tiles_n;     // partial rows holding the BN-backward sums for the next bn_bwd_finalize
    const PreReduce pre{partials, (float*)(base + w.partials2), st};
    // BatchNorm backward, step 1 for layer l (C channels, each seen nfold times in the partial rows): sums -> coefficients of
    // the data gradient + dgamma / dbeta.  Synchronised BatchNorm: the coefficients take the sums and the count of ALL ranks,
    // dgamma / dbeta this rank's own sums (the gradient all-reduce adds the ranks' parts).
    auto bwd_finalize = [&](const float* pp, int nr, double count, int l, int C, int nfold, const char* what) -> int {
        const float* local = nullptr;
        if (c->stats_allreduce) {
            if (int e = sync_row(c, pp, nr, 2 * C * nfold, base, w, st, &pp, &local)) return e;
            nr = 1;
            count *= c->stats_world;
        }
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, st, pp, nr, count, stats(l), coef, g->bn_g[l],
                           g->bn_b[l], C, nfold, local);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail((int)e, what);
    };


    T* dz = (T*)(base + w.dz);
    T* cur = (T*)(base + w.gbuf[0]);
    T* nxt = (T*)(base + w.gbuf[1]);
    bool bn_done = false;           // (see the comment above the fc loop)
    const bool fuse_ok = sizeof(T) == 2 && !opt(c, CP_OPT_UNFUSED_BN_BWD);
    // Second stream (cp_config.aux_stream, round 4): the weight gradients behind a dropout -- the projection's, fc7's + fc6's (one
    // paired launch), fc5's -- and conv2's float there beside the critical path's ~40 small launches.  Their gradient operands then
    // live in buffers of their own (w.gkeep) instead of the ping-pong, so that no data-gradient launch has to wait for them.
    // (not for the CP_OPT_FP8_BRIDGE test route, which runs this function on a CP_FP8 workspace: its gkeep buffers hold bytes)
    const Aux aux = make_aux(c, st, fuse_ok && drop && !dyn_tiles(c) && !opt(c, CP_OPT_UNPAIRED_WGRAD) && c->dtype != CP_FP8);
    float* slabs_b = (float*)(base + w.slabs_b);
    if (aux.on) { cur = (T*)(base + w.gkeep[0]); nxt = (T*)(base + w.gkeep[1]); }
    if (!(aux.on && tposed)) {              // (else made beside the forward pass and waited for by cp_encoder_backward_ev)
        if (int e = launch_weight_transposes<T>(p, base, w, st)) return e;
    }
    if (int e = aux.fork()) return e;           // dz (cp_head) is final
    // ---- projection ------------------------------------------------------------------
    {
        ProfScope ps(CP_K_PROJ_BWD, st);
        const float *s = nullptr, *t = nullptr;
        float* dzsum = (float*)(base + w.dzsum);
        if (!drop) {
            s = stats(8) + 2 * 512; t = stats(8) + 3 * 512;
            const int gb = grid_rows(N, 256 / (CP_D_E / D::EPC), 64);
            hipLaunchKernelGGL((colsum_kernel<T>), dim3(gb), dim3(256), 256 * D::EPC * 4, st, dz, partials, N, 64, CP_D_E);
            hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(CP_D_E)), dim3(FIN_THREADS), 0, st, partials, gb, CP_D_E, dzsum);  // 16 columns: tiny
            CKL("colsum(dz)");
        }
        GemmTNArgs ta{};
        const hipStream_t sw = aux.s();                 // (with dropout nothing waits for this weight gradient: second stream)
        ta.X = dz; ta.ldx = 64; ta.Y = act(8); ta.ldy = 512; ta.slabs = aux.on ? slabs_b : slabs; ta.M = N; ta.P = 64; ta.Q = 512;
        int S;
        split_rows(N, kProjSplits, &S, &ta.rows_per_split);
        const bool proj_alg = fuse_ok && drop && sizeof(T) == 2;
        if (proj_alg) {
            // behind fc7's dropout, 16-bit storage (round 4): the weight gradient's launch reads r8 ONCE and leaves both dW and fc7's
            // BatchNorm-backward sums (gemm_tn.cuh, proj_wgrad_sums_kernel); on the critical path -- the data gradient below needs the sums
            if constexpr (sizeof(T) == 2) {
                ProjWgradArgs pa{};
                pa.dz = (const bf16_t*)dz; pa.R = act(8); pa.slabs = slabs; pa.M = N; pa.rows_per_split = ta.rows_per_split; pa.splits = S;
                pa.dp_thresh = dp_thresh(c->dp_emg); pa.dp_key = dp_key(c, 8); pa.dp_salt = dp_salt(c);
                hipLaunchKernelGGL(proj_wgrad_sums_kernel<false>, dim3(PROJ_WGRAD_GRID(S)), dim3(256), 0, st, pa);
                CKL("proj_wgrad_sums_kernel");
                hipLaunchKernelGGL(proj_wgrad_finish_kernel, dim3(32, PROJ_FINISH_ROWS), dim3(256), 0, st, slabs, S, stats(8) + 2 * 512, stats(8) + 3 * 512, p->last_w,
                                   dp_inv_keep(c->dp_emg), (const int*)nullptr, g->last_w, partials);
                CKL("proj_wgrad_finish_kernel");
            }
        } else if (drop) {
            // u8 = dropout(BN(fc7)) was never written (encoder_forward_t): formed from the saved activation while staging
            ta.y_scale = stats(8) + 2 * 512; ta.y_shift = stats(8) + 3 * 512;
            ta.dp_thresh = dp_thresh(c->dp_emg); ta.dp_key = dp_key(c, 8); ta.dp_inv_keep = dp_inv_keep(c->dp_emg); ta.dp_salt = dp_salt(c);
            CK((launch_gemm_tn<T, 64, 128, YLOAD_BNDROP>(ta, S, sw)));
        } else {
            CK((launch_gemm_tn<T, 64, 128, YLOAD_PLAIN>(ta, S, sw)));
        }
        float* praw = (float*)(base + w.praw);
        if (!proj_alg) {
            hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(32), dim3(256), 0, sw, ta.slabs, S, 64, 512, CP_D_E, s, t, dzsum, g->last_w, 0,
                               drop ? (float*)nullptr : praw);
            CKL("reduce_slabs(last)");
        }
        if (!drop) {
            // BN-backward sums of fc7's BN from the projection's weight gradient (no N-sized read)
            hipLaunchKernelGGL(bn_bwd_sums_from_wgrad_kernel, dim3(512 / 64, 1), dim3(256), 0, st, praw, p->last_w, dzsum, partials,
                               CP_D_E, 512, 0);
            CKL("bn_bwd_sums_from_wgrad_kernel(last)");
            stat_rows = 1;
        }
        GemmNTArgs a{};
        a.A = dz; a.lda = 64; a.M = N; a.K = 64;
        a.W = base + w.wlast_t; a.F = 512;
        a.C = cur; a.ldc = 512; a.R = drop ? act(8) : nullptr; a.ldr = 512; a.partials = partials;
        if (drop) { a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, 8); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c); }
        int drows = 0;
        if (fuse_ok && !drop) {
            // no dropout behind fc7: its BN-backward sums are known (from the projection's weight gradient), so this
            // launch applies fc7's BN + ReLU backward itself, as the fc launches below do for their layer below
            int nr = stat_rows;
            if (int e = bwd_finalize(partials, nr, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, fused)")) return e;
            a.R = act(8); a.coef = coef; a.coef_mod = 512;
            CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, &drows, dyn_tiles(c))));
            nr = drows;
            const float* pp = pre(nr, 512);
            hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(512)), dim3(FIN_THREADS), 0, st, pp, nr, 512, g->fc_b[6]);
            CKL("colsum_finalize_kernel(fc7, fused)");
            bn_done = true;
        } else if (proj_alg) {
            // behind fc7's dropout: the rank-16 product is formed with fc7's BN + ReLU backward applied (gemm_ws.cuh, proj_dgrad_kernel)
            // instead of being written out for a separate bn_relu_bwd pass; the BatchNorm-backward sums it needs came with the weight
            // gradient above (round 3's first pass of the same product was removed; see git history)
            if (int e = bwd_finalize(partials, PROJ_FINISH_ROWS, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, projection)")) return e;
            a.coef = coef; a.coef_mod = 512;
            CK(launch_proj_dgrad(a, st, &drows));
            int nr = drows;
            const float* pp = pre(nr, 512);
            hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(512)), dim3(FIN_THREADS), 0, st, pp, nr, 512, g->fc_b[6]);
            CKL("colsum_finalize_kernel(fc7, projection)");
            bn_done = true;
        } else {
            CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, &drows, dyn_tiles(c))));
            if (drop) stat_rows = drows;             // partial rows of BN-backward sums written by this launch
        }
    }
    // ---- fc7 .. fc1 --------------------------------------------------------------------
    // bn_done: BatchNorm + ReLU backward of layer L were applied by the data-gradient launch of the layer above (its
    // staged epilogue, GemmNTArgs::coef), so `cur` already is dL/d(pre-activation) and the bias gradient is written.
    // bf16 only, and only where no dropout sits between the layers (the coefficients must exist before the launch:
    // they do when the BN-backward sums come from the weight gradient).  CP_OPT_UNFUSED_BN_BWD (cp_config.options)
    // keeps the separate pass, for the test that compares the two orders.
    struct { const T* X; const T* Y; int i; } pend{};     // a weight gradient waiting for the next layer's (see defer_wgrad)
    bool pending = false;
    for (int L = 8; L >= 2; --L) {
        const int i = L - 2, Lp = L - 1, K = fcK(i);
        if (!bn_done) {
            ProfScope ps(CP_K_BN_BWD, st);
            int nr = stat_rows;
            const float* pp = pre(nr, 2 * 512);
            if (int e = bwd_finalize(pp, nr, (double)N, L, 512, 1, "bn_bwd_finalize_kernel")) return e;
            const int gb = grid_rows(N, 256 / (512 / D::EPC), CAP_BRB16);
            hipLaunchKernelGGL((bn_relu_bwd_kernel<T>), dim3(gb), dim3(256), 256 * D::EPC * 4, st, cur, act(L), coef, partials, N, 512);
            nr = gb;
            pp = pre(nr, 512);
            // (the bias gradient is consumed within this pass -- reduce_slabs' BatchNorm un-fold and
            //  bn_bwd_sums_from_wgrad_kernel read it -- so these small launches cannot be batched at the end of the loop)
            hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(512)), dim3(FIN_THREADS), 0, st, pp, nr, 512, g->fc_b[i]);
            CKL("bn_relu_bwd_kernel");
        }
        if (int e = tap_gradient(c, L, cur, N, 512, sizeof(T), st)) return e;        // dL/d(pre-activation of layer L)
        const bool in_drop = drop && Lp >= 5;
        const T* Y = in_drop ? (const T*)(base + w.u[Lp - 5]) : act(Lp);
        const float* s = in_drop ? nullptr : stats(Lp) + 2 * kLayerC[Lp];
        const float* t = in_drop ? nullptr : stats(Lp) + 3 * kLayerC[Lp];
        int S;
        // bf16, behind a dropout: this layer's BN-backward sums do not come from its weight gradient, so nothing needs
        // the gradient before the optimiser.  fc7's and fc5's are deferred by one layer and run in ONE launch with the
        // next layer's (the gradient buffer they read is the ping-pong partner, untouched until that layer's data
        // gradient): two problems x 4 tiles x 32 splits fill the GPU with half the f32 slabs per layer (134 -> 67 MB
        // written and re-read).
        // (second stream: fc7 waits for fc6 as before -- one paired launch -- but fc5 goes alone: fc4's weight gradient is on the critical
        //  path, its product carries the BatchNorm-backward sums of the layer below)
        const bool defer_wgrad = sizeof(T) == 2 && in_drop && (i == 6 || (i == 4 && !aux.on)) && fcK(i - 1) == 512 && !opt(c, CP_OPT_UNPAIRED_WGRAD);
        const bool floats = aux.on && in_drop;           // this layer's weight gradient and slab reduction run on the second stream
        const hipStream_t sw = floats ? aux.side : st;
        float* wslabs = floats ? slabs_b : slabs;
        if (floats && !defer_wgrad) { if (int e = aux.fork()) return e; }      // cur (and the deferred layer's gradient, and both bias gradients) are final
        if (defer_wgrad) {
            pend.X = cur; pend.Y = Y; pend.i = i;
            pending = true;
        } else if constexpr (sizeof(T) == 2) {
            // 256x256 tiles: 4 (K=512) or 6 (K=768) tiles x ~256/tiles splits = one block per CU
            GemmTN256Args ta{};
            ta.X = (const bf16_t*)cur; ta.ldx = 512; ta.Y = (const bf16_t*)Y; ta.ldy = K; ta.slabs = wslabs; ta.M = N; ta.P = 512; ta.Q = K;
            if (pending) {
                ta.X2 = (const bf16_t*)pend.X; ta.Y2 = (const bf16_t*)pend.Y; ta.slabs2 = wslabs + (size_t)32 * 512 * 512;
                split_rows(N, 32, &S, &ta.rows_per_split);
            } else {
                split_rows(N, K == 512 ? 64 : 40, &S, &ta.rows_per_split);
            }
            ta.splits = S;
            ProfScope ps(CP_K_FC_WGRAD, sw);
            CK(launch_gemm_tn256(ta, sw));
        } else {
            GemmTNArgs ta{};
            ta.X = cur; ta.ldx = 512; ta.Y = Y; ta.ldy = K; ta.slabs = slabs; ta.M = N; ta.P = 512; ta.Q = K;
            split_rows(N, 32, &S, &ta.rows_per_split);
            ProfScope ps(CP_K_FC_WGRAD, st);
            CK((launch_gemm_tn<T, 128, 128, YLOAD_PLAIN>(ta, S, st)));
        }
        if (!defer_wgrad) {
            ProfScope ps(CP_K_REDUCE_SLABS, sw);
            float* praw = (float*)(base + w.praw);
            if (pending) {
                // the deferred layer (always behind a dropout: no BN fold to undo, no raw product wanted)
                hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(512), dim3(256), 0, sw, wslabs + (size_t)32 * 512 * 512, S, 512, 512, 512,
                                   (const float*)nullptr, (const float*)nullptr, g->fc_b[pend.i], g->fc_w[pend.i], 0, (float*)nullptr);
                CKL("reduce_slabs(fc, deferred)");
                pending = false;
            }
            hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(512), dim3(256), 0, sw, wslabs, S, 512, K, 512, s, t, g->fc_b[i], g->fc_w[i],
                               i == 0 ? 1 : 0, in_drop ? (float*)nullptr : praw);
            CKL("reduce_slabs(fc)");
            if (!in_drop) {
                // no dropout between this layer and the previous BN: its backward sums follow from P = g_y^T r
                // (just reduced), W and db -- the data-gradient launch below then reads no saved activation
                hipLaunchKernelGGL(bn_bwd_sums_from_wgrad_kernel, dim3(K / 64, kSumSlices), dim3(256), 0, st, praw, p->fc_w[i],
                                   g->fc_b[i], partials, 512, K, i == 0 ? 1 : 0);
                CKL("bn_bwd_sums_from_wgrad_kernel");
            }
        }
        stat_rows = in_drop ? tiles_n : kSumSlices;
        GemmNTArgs a{};
        a.A = cur; a.lda = 512; a.M = N; a.K = 512;
        a.W = base + w.wfc_t[i]; a.F = K;
        a.C = nxt; a.ldc = K; a.R = in_drop ? act(Lp) : nullptr; a.ldr = K; a.partials = partials;
        if (in_drop) { a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, Lp); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c); }
        bn_done = false;
        if (fuse_ok && !in_drop) {
            // layer Lp's BN-backward sums exist already (from the weight gradient above): finalise its coefficients
            // now and let this launch's epilogue apply BN backward + the ReLU mask to its own output tile
            const int Cp = kLayerC[Lp], nfold = K / Cp;                   // fc below: 512 x 1; conv2 below: 64 x 12
            {
                ProfScope ps(CP_K_BN_BWD, st);
                int nr = stat_rows;
                const float* pp = pre(nr, 2 * K);
                if (int e = bwd_finalize(pp, nr, (double)N * nfold, Lp, Cp, nfold, "bn_bwd_finalize_kernel(fused)")) return e;
            }
            a.R = act(Lp); a.coef = coef; a.coef_mod = Cp;
            int drows = 0;
            {
                ProfScope ps(CP_K_FC_DGRAD_BN, st);                        // data gradient + BN/ReLU backward of the layer below
                CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, &drows, dyn_tiles(c))));
            }
            if (Lp == 1) gcol_rows = drows;                               // (the conv tail reads these bias-gradient rows once more)
            {
                ProfScope ps(CP_K_BN_BWD, st);
                int nr = drows * nfold;                                   // rows of K = nfold rows of Cp
                const float* pp = pre(nr, Cp);
                float* db = Lp >= 2 ? g->fc_b[i - 1] : g->conv2_b;
                hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(Cp)), dim3(FIN_THREADS), 0, st, pp, nr, Cp, db);
                CKL("colsum_finalize_kernel(fused)");
            }
            bn_done = true;
        } else {
            // two kinds = two kernels: with input dropout the launch also reduces the BN-backward sums against
            // the saved activation (one-tile-per-block kernel), otherwise it is the persistent kernel
            ProfScope ps(in_drop ? CP_K_FC_DGRAD_STATS : CP_K_FC_DGRAD, st);
            int drows = 0;
            CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, &drows, dyn_tiles(c))));
            if (in_drop) stat_rows = drows;
        }
        if (aux.on && L >= 6) {
            // the gradients the floating launches read (layers 8, 7, 6) stay where they are; from layer 5 on the usual ping-pong
            cur = nxt;
            nxt = L == 8 ? (T*)(base + w.gkeep[2]) : (T*)(base + w.gbuf[L == 7 ? 0 : 1]);
        } else {
            T* tmp = cur; cur = nxt; nxt = tmp;
        }
    }
    return conv_backward_tail<T>(c, p, x, base, w, g, st, fc_grads_ready, cur, nxt, bn_done, stat_rows, &aux, gcol_rows);
}


// ---------------------------------------------------------------------------------------
// encoder backward, CP_FP8: the fc stack in 8 bits (csrc/fp8.cuh) -- e5m2 gradients between the layers, the saved e4m3
// activations, W^T as e4m3 -- then the conv stack on the bf16 kernels (fc1's data-gradient launch writes bf16).
// Same order of work as encoder_backward_t<bf16_t>; CPNATIVE_FP8_BRIDGE keeps the first build's route (expand the saved
// tensors to bf16, run the bf16 backward) for A/B runs and for the test that compares the two.
// ---------------------------------------------------------------------------------------
static int encoder_backward_fp8(const cp_config* c, const cp_params* p, const float* x, unsigned char* base, const WS& w,
                                cp_params* g, hipStream_t st, hipEvent_t fc_grads_ready, bool tposed = false) {
    using T = bf16_t;
    const int64_t N = c->n_windows;
    const bool drop = c->training && c->dp_emg > 0.f;
    float* partials = (float*)(base + w.partials);
    float* slabs = (float*)(base + w.slabs);
    float* coef = (float*)(base + w.coef);
    float* praw = (float*)(base + w.praw);
    Fp8State* fs = (Fp8State*)(base + w.f8state);
    auto stats = [&](int l) { return (float*)(base + w.stats[l]); };
    const PreReduce pre{partials, (float*)(base + w.partials2), st};
    auto bwd_finalize = [&](const float* pp, int nr, double count, int l, int C, int nfold, const char* what) -> int {
        const float* local = nullptr;
        if (c->stats_allreduce) {          // synchronised BatchNorm (these sums are in true units on this path)
            if (int e = sync_row(c, pp, nr, 2 * C * nfold, base, w, st, &pp, &local)) return e;
            nr = 1;
            count *= c->stats_world;
        }
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, st, pp, nr, count, stats(l), coef, g->bn_g[l],
                           g->bn_b[l], C, nfold, local);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail((int)e, what);
    };
    auto tap8 = [&](int slot, const uint8_t* src, int t) -> int {          // test aid: the e5m2 gradient expanded into the bf16 tap
        if (!c->grad_tap) return 0;
        const size_t slot_bytes = (size_t)N * 768 * 2;
        if ((size_t)(slot + 1) * slot_bytes > c->grad_tap_bytes) return fail(CP_ERR_ARG, "gradient tap buffer too small");
        hipLaunchKernelGGL(dequant5_bf16_kernel, dim3(1024), dim3(256), 0, st, src, (bf16_t*)((unsigned char*)c->grad_tap + slot * slot_bytes), N * 128, fs, t);
        CKL("dequant5_bf16_kernel");
        return 0;
    };
    T* dz = (T*)(base + w.dz);
    uint8_t* cur = base + w.g8[0];
    uint8_t* nxt = base + w.g8[1];
    int stat_rows = 0, gcol_rows = 0;
    bool bn_done = false;
    // second stream (encoder_backward_t): the projection's, fc7's + fc6's and fc5's weight gradients float beside the critical path
    const Aux aux = make_aux(c, st, drop);
    float* slabs_b = (float*)(base + w.slabs_b);
    if (aux.on) { cur = base + w.gkeep[0]; nxt = base + w.gkeep[1]; }
    if (!(aux.on && tposed)) {
        if (int e = launch_weight_transposes_fp8(p, base, w, st)) return e;
    }
    if (int e = aux.fork()) return e;
    // ---- projection ------------------------------------------------------------------
    {
        ProfScope ps(CP_K_PROJ_BWD, st);
        float* dzsum = (float*)(base + w.dzsum);
        const float *s = nullptr, *t = nullptr;
        if (!drop) {
            s = stats(8) + 2 * 512; t = stats(8) + 3 * 512;
            const int gb = grid_rows(N, 256 / (CP_D_E / DT<T>::EPC), 64);
            hipLaunchKernelGGL((colsum_kernel<T>), dim3(gb), dim3(256), 256 * DT<T>::EPC * 4, st, dz, partials, N, 64, CP_D_E);
            hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(CP_D_E)), dim3(FIN_THREADS), 0, st, partials, gb, CP_D_E, dzsum);
            CKL("colsum(dz)");
        }
        GemmTNArgs ta{};
        const hipStream_t sw = aux.s();
        ta.X = dz; ta.ldx = 64; ta.Y = base + w.act8[8]; ta.ldy = 512; ta.slabs = aux.on ? slabs_b : slabs; ta.M = N; ta.P = 64; ta.Q = 512;
        ta.y_exp = &fs->e[F8_T_ACT + 8];
        int S;
        split_rows(N, kProjSplits, &S, &ta.rows_per_split);
        if (drop) {
            // (encoder_backward_t: one pass over r8 for the weight gradient AND fc7's BatchNorm-backward sums, on the critical path)
            ProjWgradArgs pa{};
            pa.dz = (const bf16_t*)dz; pa.R = base + w.act8[8]; pa.slabs = slabs; pa.M = N; pa.rows_per_split = ta.rows_per_split; pa.splits = S;
            pa.dp_thresh = dp_thresh(c->dp_emg); pa.dp_key = dp_key(c, 8); pa.dp_salt = dp_salt(c);
            hipLaunchKernelGGL(proj_wgrad_sums_kernel<true>, dim3(PROJ_WGRAD_GRID(S)), dim3(256), 0, st, pa);
            CKL("proj_wgrad_sums_kernel<e4m3>");
            hipLaunchKernelGGL(proj_wgrad_finish_kernel, dim3(32, PROJ_FINISH_ROWS), dim3(256), 0, st, slabs, S, stats(8) + 2 * 512, stats(8) + 3 * 512, p->last_w,
                               dp_inv_keep(c->dp_emg), (const int*)&fs->e[F8_T_ACT + 8], g->last_w, partials);
            CKL("proj_wgrad_finish_kernel");
        } else {
            CK((launch_gemm_tn<T, 64, 128, YLOAD_F8>(ta, S, sw)));
            hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(32), dim3(256), 0, sw, ta.slabs, S, 64, 512, CP_D_E, s, t, dzsum, g->last_w, 0, praw,
                               (const int*)nullptr, (const int*)nullptr);
            CKL("reduce_slabs(last)");
        }
        Proj8Args a{};
        a.A = dz; a.lda = 64; a.W = (const bf16_t*)(base + w.wlast_t); a.K = 64; a.R = base + w.act8[8]; a.C = cur;
        a.partials = partials; a.st = fs; a.t_r = F8_T_ACT + 8; a.t_out = F8_T_GRAD + 8; a.M = N;
        int drows = 0;
        if (drop) {
            a.dp_thresh = dp_thresh(c->dp_emg); a.dp_key = dp_key(c, 8); a.dp_inv_keep = dp_inv_keep(c->dp_emg); a.dp_salt = dp_salt(c);
            if (int e = bwd_finalize(partials, PROJ_FINISH_ROWS, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, projection)")) return e;
        } else {
            // no dropout behind fc7: its BatchNorm-backward sums follow from the projection's weight gradient (no N-sized read)
            hipLaunchKernelGGL(bn_bwd_sums_from_wgrad_kernel, dim3(512 / 64, 1), dim3(256), 0, st, praw, p->last_w, dzsum, partials, CP_D_E, 512, 0);
            CKL("bn_bwd_sums_from_wgrad_kernel(last)");
            if (int e = bwd_finalize(partials, 1, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, fused)")) return e;
        }
        a.coef = coef;
        CK(launch_proj_dgrad8(a, st, &drows));
        int nr = drows;
        const float* pp = pre(nr, 512);
        hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(512)), dim3(FIN_THREADS), 0, st, pp, nr, 512, g->fc_b[6]);
        CKL("colsum_finalize_kernel(fc7)");
        bn_done = true;
    }
    // ---- fc7 .. fc1 --------------------------------------------------------------------
    struct { const uint8_t* X; const uint8_t* Y; int i, tx, ty; } pend{};
    bool pending = false;
    T* gconv = (T*)(base + w.gbuf[0]);                       // fc1's data gradient, e5m2 [N][768] (F8_T_GRAD + 1): what the conv kernels read
    for (int L = 8; L >= 2; --L) {
        const int i = L - 2, Lp = L - 1, K = fcK(i);
        if (!bn_done) {
            // cur = masked dL/d(BN_L output) (F8_T_GB + L): BatchNorm + ReLU backward in place -> dL/d(pre-activation) (F8_T_GRAD + L)
            ProfScope ps(CP_K_BN_BWD, st);
            int nr = stat_rows;
            const float* pp = pre(nr, 2 * 512);
            if (int e = bwd_finalize(pp, nr, (double)N, L, 512, 1, "bn_bwd_finalize_kernel")) return e;
            const int gb = grid_rows(N, 256 / (512 / 16), CAP_BRB8);
            hipLaunchKernelGGL(bn_relu_bwd8_kernel, dim3(gb), dim3(256), 8 * 512 * 4, st, cur, base + w.act8[L], coef, partials, N, 512, fs,
                               F8_T_GB + L, F8_T_ACT + L, F8_T_GRAD + L);
            nr = gb;
            pp = pre(nr, 512);
            hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(512)), dim3(FIN_THREADS), 0, st, pp, nr, 512, g->fc_b[i]);
            CKL("bn_relu_bwd8_kernel");
        }
        if (int e = tap8(L, cur, F8_T_GRAD + L)) return e;
        const bool in_drop = drop && Lp >= 5;
        const uint8_t* Y = in_drop ? base + w.u8[Lp - 5] : base + w.act8[Lp];
        const int ty = in_drop ? F8_T_U + (Lp - 5) : F8_T_ACT + Lp, tx = F8_T_GRAD + L;
        const float* s = in_drop ? nullptr : stats(Lp) + 2 * kLayerC[Lp];
        const float* t = in_drop ? nullptr : stats(Lp) + 3 * kLayerC[Lp];
        int S;
        const bool defer_wgrad = in_drop && (i == 6 || (i == 4 && !aux.on)) && fcK(i - 1) == 512;
        const bool floats = aux.on && in_drop;
        const hipStream_t sw = floats ? aux.side : st;
        float* wslabs = floats ? slabs_b : slabs;
        if (floats && !defer_wgrad) { if (int e = aux.fork()) return e; }
        if (defer_wgrad) {
            pend.X = cur; pend.Y = Y; pend.i = i; pend.tx = tx; pend.ty = ty;
            pending = true;
        } else {
            GemmTN8Args ta{};
            ta.X = cur; ta.ldx = 512; ta.Y = Y; ta.ldy = K; ta.slabs = wslabs; ta.M = N; ta.P = 512; ta.Q = K;
            // (32 splits for the single-layer launches too -- half the slab bytes, half the blocks -- measured: weight gradients 5 x 67 -> 82 us,
            //  slab reductions 9 x 11.0 -> 9.1: 70 us lost for 17 gained)
            const int target = pending ? 32 : (K == 512 ? 64 : 40);
            int64_t rps = (N + target - 1) / target;
            rps = ((rps + 63) / 64) * 64;
            ta.rows_per_split = rps;
            S = (int)((N + rps - 1) / rps);
            if (pending) { ta.X2 = pend.X; ta.Y2 = pend.Y; ta.slabs2 = wslabs + (size_t)32 * 512 * 512; }
            ta.splits = S;
            ProfScope ps(CP_K_FC_WGRAD, sw);
            CK(launch_gemm_tn8(ta, sw));
        }
        if (!defer_wgrad) {
            ProfScope ps(CP_K_REDUCE_SLABS, sw);
            if (pending) {
                hipLaunchKernelGGL(reduce_slabs_kernel<bf16_t>, dim3(512), dim3(256), 0, sw, wslabs + (size_t)32 * 512 * 512, S, 512, 512, 512,
                                   (const float*)nullptr, (const float*)nullptr, g->fc_b[pend.i], g->fc_w[pend.i], 0, (float*)nullptr,
                                   (const int*)&fs->e[pend.tx], (const int*)&fs->e[pend.ty]);
                CKL("reduce_slabs(fc, deferred)");
                pending = false;
            }
            hipLaunchKernelGGL(reduce_slabs_kernel<bf16_t>, dim3(512), dim3(256), 0, sw, wslabs, S, 512, K, 512, s, t, g->fc_b[i], g->fc_w[i],
                               i == 0 ? 1 : 0, in_drop ? (float*)nullptr : praw, (const int*)&fs->e[tx], (const int*)&fs->e[ty]);
            CKL("reduce_slabs(fc)");
            if (!in_drop) {
                hipLaunchKernelGGL(bn_bwd_sums_from_wgrad_kernel, dim3(K / 64, kSumSlices), dim3(256), 0, st, praw, p->fc_w[i], g->fc_b[i],
                                   partials, 512, K, i == 0 ? 1 : 0);
                CKL("bn_bwd_sums_from_wgrad_kernel");
            }
        }
        Wsd8Args a{};
        a.A = cur; a.W = base + w.wfc8t[i]; a.wsc = base + w.wsc8t[i]; a.R = base + w.act8[Lp]; a.partials = partials;
        a.st = fs; a.t_r = F8_T_ACT + Lp; a.M = N; a.F = K;
        bn_done = false;
        if (!in_drop) {
            const int Cp = kLayerC[Lp], nfold = K / Cp;
            {
                ProfScope ps(CP_K_BN_BWD, st);
                int nr = kSumSlices;
                const float* pp = pre(nr, 2 * K);
                if (int e = bwd_finalize(pp, nr, (double)N * nfold, Lp, Cp, nfold, "bn_bwd_finalize_kernel(fused)")) return e;
            }
            a.coef = coef; a.coef_mod = Cp;
            int drows = 0;
            {
                ProfScope ps(Lp == 1 ? CP_K_FC_DGRAD_CONV : CP_K_FC_DGRAD_BN, st);
                // (fc1's launch writes e5m2 like the others -- round 3's wrote 258 MB of bf16 for the conv kernels; they expand the bytes now)
                a.C = Lp == 1 ? (void*)gconv : (void*)nxt; a.t_out = F8_T_GRAD + Lp;
                CK((launch_gemm_wsd8<0>(a, st, &drows)));
                if (Lp == 1) gcol_rows = drows;
            }
            {
                ProfScope ps(CP_K_BN_BWD, st);
                int nr = drows * nfold;
                const float* pp = pre(nr, Cp);
                float* db = Lp >= 2 ? g->fc_b[i - 1] : g->conv2_b;
                hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(Cp)), dim3(FIN_THREADS), 0, st, pp, nr, Cp, db);
                CKL("colsum_finalize_kernel(fused)");
            }
            bn_done = true;
        } else {
            // (the dropout OUTPUT of layer Lp stands in for its saved activation: its zeros are the mask -- fp8.cuh, MODE 1)
            a.C = nxt; a.t_out = F8_T_GB + Lp;
            a.R = base + w.u8[Lp - 5]; a.t_r = F8_T_U + (Lp - 5); a.bn_stats = stats(Lp); a.dp_inv_keep = dp_inv_keep(c->dp_emg);
            ProfScope ps(CP_K_FC_DGRAD_STATS, st);
            int drows = 0;
            CK((launch_gemm_wsd8<1>(a, st, &drows)));
            stat_rows = drows;
        }
        if (aux.on && L >= 6) {
            cur = nxt;
            nxt = L == 8 ? base + w.gkeep[2] : base + w.g8[L == 7 ? 0 : 1];
        } else {
            uint8_t* tmp = cur; cur = nxt; nxt = tmp;
        }
    }
    return conv_backward_tail<T>(c, p, x, base, w, g, st, fc_grads_ready, gconv, (T*)(base + w.gbuf[1]), true, 0, &aux, gcol_rows, fs);
}

extern "C" int cp_encoder_backward_ev(const cp_config* cfg, const cp_params* p, const float* x, void* ws, size_t ws_bytes,
                                      cp_params* grads, void* stream, void* fc_grads_ready) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (!p || !x || !grads) return fail(CP_ERR_ARG, "cp_encoder_backward args");
    if (((uintptr_t)x & 15) != 0) return fail(CP_ERR_ARG, "x must be 16-byte aligned");
    cp_forward_record* r = cfg->record;
    if (!r) return fail(CP_ERR_ARG, "cp_encoder_backward: cfg->record is NULL (pass the record cp_encoder_forward filled)");
    if (!r->n_windows) return fail(CP_ERR_ARG, "cp_encoder_backward: no cp_encoder_forward has filled cfg->record");
    // the path is the FORWARD's: use_small() ignores `training`, which a backward call may not carry, only through (training || adabn)
    if (r->n_windows != cfg->n_windows || r->path != forward_path(cfg))
        return fail(CP_ERR_ARG, "cp_encoder_backward: n_windows or the kernel path differs from the forward pass that filled cfg->record");
    const int repeats = r->backwards++;
    const bool tposed = r->transposed != 0;
    // the transposed weights made beside the forward pass (cp_encoder_forward) precede every launch of this call, whether or not this
    // call uses the second stream itself
    if (tposed) CK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)r->join_event, 0));
    if (cfg->dtype != CP_FP8 && use_small(cfg)) {
        if (repeats > 0) {
            // a second backward over the same forward: the small-batch form's BatchNorm-backward totals (fixed-point atomics, zeroed by the
            // forward's preparation launch) already hold the first pass's sums
            CK(hipMemsetAsync((unsigned char*)ws + w.sm_acc + (size_t)9 * 2 * 768 * 8, 0, (size_t)9 * 2 * 768 * 8, (hipStream_t)stream));
        }
        if (cfg->dtype == CP_BF16)
            return encoder_backward_small_t<bf16_t>(cfg, p, x, (unsigned char*)ws, w, grads, (hipStream_t)stream, (hipEvent_t)fc_grads_ready);
        return encoder_backward_small_t<float>(cfg, p, x, (unsigned char*)ws, w, grads, (hipStream_t)stream, (hipEvent_t)fc_grads_ready);
    }
    if (cfg->dtype == CP_FP8 && !opt(cfg, CP_OPT_FP8_BRIDGE))
        return encoder_backward_fp8(cfg, p, x, (unsigned char*)ws, w, grads, (hipStream_t)stream, (hipEvent_t)fc_grads_ready, tposed);
    if (cfg->dtype == CP_FP8) {
        // (bridge = the first build's route, kept for A/B runs and as the test's comparison: the e4m3 tensors of the forward pass are
        //  expanded to bf16 -- exactly -- and the bf16 backward kernels run on them)
        unsigned char* base = (unsigned char*)ws;
        hipStream_t st = (hipStream_t)stream;
        const Fp8State* fs = (const Fp8State*)(base + w.f8state);
        const int64_t N = cfg->n_windows;
        const bool drop = cfg->training && cfg->dp_emg > 0.f;
        for (int l = 1; l < CP_N_BN; ++l) {
            const int64_t n16 = N * (l < 2 ? 768 : 512) / 16;
            hipLaunchKernelGGL(dequant8_bf16_kernel, dim3(grid_rows(n16, 256, 4096)), dim3(256), 0, st, base + w.act8[l], (bf16_t*)(base + w.act[l]), n16, fs, F8_T_ACT + l);
        }
        if (drop)
            for (int i = 0; i < 3; ++i)
                hipLaunchKernelGGL(dequant8_bf16_kernel, dim3(grid_rows(N * 32, 256, 4096)), dim3(256), 0, st, base + w.u8[i], (bf16_t*)(base + w.u[i]), N * 32, fs, F8_T_U + i);
        CKL("dequant8_bf16_kernel");
        return encoder_backward_t<bf16_t>(cfg, p, x, base, w, grads, st, (hipEvent_t)fc_grads_ready);
    }
    if (cfg->dtype == CP_BF16)
        return encoder_backward_t<bf16_t>(cfg, p, x, (unsigned char*)ws, w, grads, (hipStream_t)stream, (hipEvent_t)fc_grads_ready, tposed);
    return encoder_backward_t<float>(cfg, p, x, (unsigned char*)ws, w, grads, (hipStream_t)stream, (hipEvent_t)fc_grads_ready);
}

extern "C" int cp_encoder_backward(const cp_config* cfg, const cp_params* p, const float* x, void* ws, size_t ws_bytes,
                                   cp_params* grads, void* stream) {
    return cp_encoder_backward_ev(cfg, p, x, ws, ws_bytes, grads, stream, nullptr);
}

// ---------------------------------------------------------------------------------------
// optimiser
// ---------------------------------------------------------------------------------------
static int build_opt(OptArgs* a, const int64_t* off, const int64_t* numel, const int32_t* group, const int32_t* l2, int n) {
    if (n <= 0 || n > CP_MAX_TENSORS || !off || !numel || !group || !l2) return fail(CP_ERR_ARG, "tensor table");
    int chunk = 0;
    for (int i = 0; i < n; ++i) {
        a->t[i].offset = off[i];
        a->t[i].numel = numel[i];
        a->t[i].chunk0 = chunk;
        a->t[i].nchunks = (int)((numel[i] + OPT_CHUNK - 1) / OPT_CHUNK);
        a->t[i].group = group[i] ? 1 : 0;
        a->t[i].l2 = l2[i] ? 1 : 0;
        chunk += a->t[i].nchunks;
    }
    a->n_tensors = n;
    a->total_chunks = chunk;
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
    if (int e = build_opt(&a, offset_host, numel_host, group_host, l2_host, n)) return e;
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
    if (int e = build_opt(&a, offset_host, numel_host, group_host, l2_host, n)) return e;
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
    if (int e = build_opt(&a, offset_host, numel_host, group_host, l2_host, n)) return e;
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
__global__ void to_f32_kernel(const T* __restrict__ in, float* __restrict__ out, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = DT<T>::load(in + i);
}

extern "C" int cp_debug_activation(const cp_config* cfg, const cp_params* p, const float* x, void* ws, size_t ws_bytes,
                                   int32_t layer, float* out, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (layer < 0 || layer >= CP_N_BN + 4 || !out) return fail(CP_ERR_ARG, "cp_debug_activation args");
    if (layer >= CP_N_BN && !(cfg->dp_emg > 0.f)) return fail(CP_ERR_ARG, "dropout buffers exist only when dp_emg > 0");
    const int64_t n = cfg->n_windows * (layer < 2 ? 768 : 512);
    unsigned char* base = (unsigned char*)ws;
    if (layer == 0) {   // conv1's output is never stored: recompute it exactly as its consumers do
        if (!p || !x) return fail(CP_ERR_ARG, "layer 0 needs params and x");
        const int64_t rows = cfg->n_windows * 12;
        if (cfg->dtype != CP_F32)
            hipLaunchKernelGGL((conv1_materialize_kernel<bf16_t>), dim3(1024), dim3(256), 0, (hipStream_t)stream, x, p->conv1_w,
                               p->conv1_b, out, rows);
        else
            hipLaunchKernelGGL((conv1_materialize_kernel<float>), dim3(1024), dim3(256), 0, (hipStream_t)stream, x, p->conv1_w,
                               p->conv1_b, out, rows);
        CKL("conv1_materialize_kernel");
        return 0;
    }
    if (cfg->dtype == CP_FP8) {
        // the stored e4m3 tensor in true units (dropout(BN(fc7)), layer CP_N_BN + 3, is never stored on this path)
        if (layer == CP_N_BN + 3) {
            // dropout(BN(fc7)) is formed while staging and never stored: computed here in f32 from the stored e4m3 activation, same key
            hipLaunchKernelGGL(debug_bn_dropout8_f32_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, base + w.act8[8],
                               (const float*)(base + w.stats[8]), out, cfg->n_windows, 512, dp_thresh(cfg->dp_emg), dp_key(cfg, 8),
                               dp_inv_keep(cfg->dp_emg), dp_salt(cfg), (const Fp8State*)(base + w.f8state), F8_T_ACT + 8);
            CKL("debug_bn_dropout8_f32_kernel");
            return 0;
        }
        const int t = layer < CP_N_BN ? F8_T_ACT + layer : F8_T_U + (layer - CP_N_BN);
        const uint8_t* src = base + (layer < CP_N_BN ? w.act8[layer] : w.u8[layer - CP_N_BN]);
        hipLaunchKernelGGL(dequant8_f32_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, src, out, n, (const Fp8State*)(base + w.f8state), t);
        CKL("dequant8_f32_kernel");
        return 0;
    }
    const size_t off = layer < CP_N_BN ? w.act[layer] : w.u[layer - CP_N_BN];
    // dropout(BN(.)) of fc4..fc6 is STORED by the large-batch forward: read what it stored.  fc7's (formed while staging, never
    // written) and all four after a small-batch forward (csrc/small.cuh applies BatchNorm + dropout while staging) are recomputed from
    // the stored activation with the forward pass's key, into the otherwise unused buffer.
    const bool stored_u = layer >= CP_N_BN && layer < CP_N_BN + 3 &&
                          (cfg->record && cfg->record->n_windows ? cfg->record->path : forward_path(cfg)) == PATH_LARGE;
    if (layer >= CP_N_BN && !stored_u) {
        const int Lp = 5 + (layer - CP_N_BN);
        const int64_t N = cfg->n_windows;
        const float* stp = (const float*)(base + w.stats[Lp]);
        if (cfg->dtype == CP_BF16)
            hipLaunchKernelGGL((bn_dropout_apply_kernel<bf16_t>), dim3(grid_rows(N, 256 / (512 / 8), 4096)), dim3(256), 0, (hipStream_t)stream,
                               (const bf16_t*)(base + w.act[Lp]), stp, (bf16_t*)(base + off), N, 512, dp_thresh(cfg->dp_emg), dp_key(cfg, Lp),
                               dp_inv_keep(cfg->dp_emg), dp_salt(cfg));
        else
            hipLaunchKernelGGL((bn_dropout_apply_kernel<float>), dim3(grid_rows(N, 256 / (512 / 4), 4096)), dim3(256), 0, (hipStream_t)stream,
                               (const float*)(base + w.act[Lp]), stp, (float*)(base + off), N, 512, dp_thresh(cfg->dp_emg), dp_key(cfg, Lp),
                               dp_inv_keep(cfg->dp_emg), dp_salt(cfg));
        CKL("bn_dropout_apply_kernel(debug)");
    }
    if (cfg->dtype == CP_BF16)
        hipLaunchKernelGGL((to_f32_kernel<bf16_t>), dim3(1024), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)(base + off), out, n);
    else
        hipLaunchKernelGGL((to_f32_kernel<float>), dim3(1024), dim3(256), 0, (hipStream_t)stream, (const float*)(base + off), out, n);
    CKL("to_f32_kernel");
    return 0;
}

template <typename T>
static int debug_gemm_t(int kind, int64_t M, int K, int F, const void* A, const void* W, void* C, const float* bias,
                        const void* R, float* partials, hipStream_t st) {
    if (kind == 2) {
        int S;
        if constexpr (sizeof(T) == 2) {
            GemmTN256Args ta{};
            ta.X = (const bf16_t*)A; ta.ldx = K; ta.Y = (const bf16_t*)W; ta.ldy = F; ta.slabs = (float*)C; ta.M = M; ta.P = K; ta.Q = F;
            split_rows(M, F == 512 ? 64 : 40, &S, &ta.rows_per_split);
            ta.splits = S;
            CK(launch_gemm_tn256(ta, st));
        } else {
            GemmTNArgs ta{};
            ta.X = A; ta.ldx = K; ta.Y = W; ta.ldy = F; ta.slabs = (float*)C; ta.M = M; ta.P = K; ta.Q = F;
            split_rows(M, 32, &S, &ta.rows_per_split);
            CK((launch_gemm_tn<T, 128, 128, YLOAD_PLAIN>(ta, S, st)));
        }
        return 0;
    }
    GemmNTArgs a{};
    a.A = A; a.lda = K; a.M = M; a.K = K; a.W = W; a.F = F; a.C = C; a.ldc = F; a.bias = bias; a.relu = 1;
    a.R = R; a.ldr = F; a.partials = partials;
    if (kind == 0) CK((launch_fc_gemm<T, EPI_FWD>(a, st)));
    else CK((launch_fc_gemm<T, EPI_DGRAD>(a, st)));
    return 0;
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
    if (dtype == CP_BF16) return debug_gemm_t<bf16_t>(kind, M, K, F, A, W, C, bias, R, partials, (hipStream_t)stream);
    return debug_gemm_t<float>(kind, M, K, F, A, W, C, bias, R, partials, (hipStream_t)stream);
}

extern "C" int cp_debug_bn_stats(const cp_config* cfg, void* ws, size_t ws_bytes, int32_t layer, float* out, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (layer < 0 || layer >= CP_N_BN || !out) return fail(CP_ERR_ARG, "cp_debug_bn_stats args");
    CK(hipMemcpyAsync(out, (unsigned char*)ws + w.stats[layer], (size_t)4 * kLayerC[layer] * 4, hipMemcpyDeviceToDevice,
                      (hipStream_t)stream));
    return 0;
}

#include "online_api.cuh"             // the cp_online_* entries: host layer of the online decoders, the gate and the gate sweep
