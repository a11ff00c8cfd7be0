// Host layer of the training encoder: the workspace of cp_encoder_forward / cp_encoder_backward, the launch helpers, the forward and
// backward pass in their three forms (16/32-bit large batch, CP_FP8, small batch) built from shared pieces, the entry points, and the
// debug readers of the same workspace.  Host code only; api.hip includes it behind its own helpers (fail, CK, CKL, opt, dyn_tiles,
// ProfScope, to_f32_kernel), so the library stays one translation unit.
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

// the projection's weights as its launches read them, from the reference layout Wp (16, 512) f32 (the caller checks the launch):
// wlast[32][512] T = Wp diag s (s NULL: the plain copy) with rows 16..31 zero and blast[16] = Wp t, for the forward launch;
// wlast_t[512][64] T = Wp^T with columns 16..63 zero, for the data gradient
template <typename T>
static inline void launch_proj_fold(const float* Wp, const float* s, const float* t, void* wlast, float* blast, hipStream_t st) {
    hipLaunchKernelGGL((fold_linear_kernel<T>), dim3(32), dim3(256), 0, st, Wp, (const float*)nullptr, s, t, (T*)wlast, blast, CP_D_E, 512, 0);
}
template <typename T>
static inline void launch_proj_transpose(const float* Wp, void* wlast_t, hipStream_t st) {
    hipLaunchKernelGGL((transpose_w_kernel<T>), dim3(64), dim3(256), 0, st, Wp, (T*)wlast_t, CP_D_E, 512, 64, 0);
}

// the transposed weights the data-gradient launches read: fc1..fc7 and the projection (bf16 / f32), their e4m3 form + the projection's
// (CP_FP8).  Made once per step: at the start of the backward pass, or -- second stream -- beside the forward pass.
// where the weight preparation launches put what they make: the images in the compute dtype and the f32 biases of fc1..fc7 and the
// projection, and the transposed images.  The step fills it from its workspace (prep_images), cp_debug_bn from caller buffers: both
// reach the batched kernels through the launch functions that take it (launch_weight_transposes here; launch_eval_folds,
// launch_fold_copies below), with their job tables and grids
struct PrepImages {
    void* wfc[CP_N_FC]; float* bfc[CP_N_FC]; void* wlast; float* blast;
    void* wfc_t[CP_N_FC]; void* wlast_t;
};
static inline PrepImages prep_images(unsigned char* base, const WS& w) {
    PrepImages im{};
    for (int i = 0; i < CP_N_FC; ++i) { im.wfc[i] = base + w.wfc[i]; im.bfc[i] = (float*)(base + w.bfc[i]); im.wfc_t[i] = base + w.wfc_t[i]; }
    im.wlast = base + w.wlast; im.blast = (float*)(base + w.blast); im.wlast_t = base + w.wlast_t;
    return im;
}
template <typename T>
static int launch_weight_transposes(const cp_params* p, const PrepImages& im, hipStream_t st) {
    TransposeBatch tb{};
    for (int i = 0; i < CP_N_FC; ++i) tb.job[i] = TransposeJob{p->fc_w[i], im.wfc_t[i], 512, fcK(i), 512, i == 0 ? 1 : 0};
    tb.job[CP_N_FC] = TransposeJob{p->last_w, im.wlast_t, CP_D_E, 512, 64, 0};
    hipLaunchKernelGGL((transpose_w_batch_kernel<T>), dim3(128, CP_N_FC + 1), dim3(256), 0, st, tb);
    CKL("transpose_w_batch_kernel");
    return 0;
}
template <typename T>
static int launch_weight_transposes(const cp_params* p, unsigned char* base, const WS& w, hipStream_t st) {
    ProfScope ps(CP_K_PREP, st);
    return launch_weight_transposes<T>(p, prep_images(base, w), st);
}
// the 8-bit weight preparation launches (cp_debug_fp8 runs the same two on one layer): one block per output row of a fold; 12 column
// blocks of 64 (K <= 768) x jobs x 4 row quarters of a transpose
static inline void launch_fold_linear8(const float* W, const float* b, const float* s, const float* t, uint8_t* out_w, uint8_t* out_sc, float* out_b,
                                       int K, int mode, const Fp8State* fs, int t_in, int t_out, hipStream_t st) {
    hipLaunchKernelGGL(fold_linear8_kernel, dim3(512), dim3(256), 0, st, W, b, s, t, out_w, out_sc, out_b, K, mode, fs, t_in, t_out);
}
static inline void launch_transpose_w8_batch(const Transpose8Batch& tb, int jobs, const Fp8State* fs, hipStream_t st) {
    hipLaunchKernelGGL(transpose_w8_batch_kernel, dim3(12, jobs, 4), dim3(256), 0, st, tb, fs);
}
static int launch_weight_transposes_fp8(const cp_params* p, unsigned char* base, const WS& w, hipStream_t st) {
    ProfScope ps(CP_K_PREP, st);
    const Fp8State* fs = (const Fp8State*)(base + w.f8state);
    Transpose8Batch tb{};
    for (int i = 0; i < CP_N_FC; ++i)
        tb.job[i] = Transpose8Job{p->fc_w[i], base + w.wfc8t[i], base + w.wsc8t[i], fcK(i), i == 0 ? 1 : 0, F8_T_GRAD + (i + 2)};
    launch_transpose_w8_batch(tb, CP_N_FC, fs, st);
    launch_proj_transpose<bf16_t>(p->last_w, base + w.wlast_t, st);
    CKL("transpose kernels (fp8)");
    return 0;
}

// ---------------------------------------------------------------------------------------
// launch helpers
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

// The 8-bit streaming passes around a dropout as the step launches them (cp_debug_fp8 runs the same functions on caller buffers):
// 512 features, 8 rows per block.  launch_bn_relu_bwd8 returns the number of partial rows (= its grid).
static inline void launch_bn_dropout_apply8(const uint8_t* r, const float* stats, uint8_t* u, int64_t N, uint32_t thresh, uint32_t key, float inv_keep,
                                            const uint32_t* salt, Fp8State* fs, int t_in, int t_out, hipStream_t st) {
    hipLaunchKernelGGL(bn_dropout_apply8_kernel, dim3(grid_rows(N, 256 / (512 / 16), CAP_BDA8)), dim3(256), 0, st, r, stats, u, N, 512,
                       thresh, key, inv_keep, salt, fs, t_in, t_out);
}
static inline int launch_bn_relu_bwd8(uint8_t* g, const uint8_t* r, const float* coef, float* partials, int64_t N, Fp8State* fs, int t_in, int t_r,
                                      int t_out, hipStream_t st) {
    const int gb = grid_rows(N, 256 / (512 / 16), CAP_BRB8);
    hipLaunchKernelGGL(bn_relu_bwd8_kernel, dim3(gb), dim3(256), 8 * 512 * 4, st, g, r, coef, partials, N, 512, fs, t_in, t_r, t_out);
    return gb;
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
        if (a.bn_rows) return hipErrorInvalidValue;          // (only that kernel forms its coefficients itself)
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

// The f32 / bf16 BatchNorm launches between the GEMMs as the step makes them (cp_debug_bn runs the same functions on caller buffers;
// the caller checks the launch).  launch_bn_relu_bwd returns the number of partial rows (= its grid); `cap`: CAP_BRB16 at C = 512,
// 2,048 at C = 64 (conv2's BatchNorm, rows = windows * 12).
static inline void launch_bn_finalize(const float* pp, int nrows, double count, const float* gamma, const float* beta, float* running_mean,
                                      float* running_var, int update_running, float momentum, float eps, float* stats, int C, const int* unscale,
                                      hipStream_t st) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, st, pp, nrows, count, gamma, beta, running_mean, running_var,
                       update_running, 0, momentum, eps, stats, C, unscale);
}
static inline void launch_bn_bwd_finalize(const float* pp, int nr, double count, const float* stats, float* coef, float* dgamma, float* dbeta, int C,
                                          int nfold, const float* local, hipStream_t st) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, st, pp, nr, count, stats, coef, dgamma, dbeta, C, nfold, local);
}
template <typename T>
static inline void launch_bn_dropout_apply(const T* r, const float* stats, T* u, int64_t N, uint32_t thresh, uint32_t key, float inv_keep,
                                           const uint32_t* salt, hipStream_t st) {
    hipLaunchKernelGGL((bn_dropout_apply_kernel<T>), dim3(grid_rows(N, 256 / (512 / DT<T>::EPC), CAP_BDA16)), dim3(256), 0, st, r, stats, u, N, 512,
                       thresh, key, inv_keep, salt);
}
template <typename T>
static inline int launch_bn_relu_bwd(T* g, const T* r, const float* coef, float* partials, int64_t rows, int C, int cap, hipStream_t st) {
    using D = DT<T>;
    const int gb = grid_rows(rows, 256 / (C / D::EPC), cap);
    hipLaunchKernelGGL((bn_relu_bwd_kernel<T>), dim3(gb), dim3(256), 256 * D::EPC * 4, st, g, r, coef, partials, rows, C);
    return gb;
}
// a bias gradient = the column sums of `rows` partial rows of C floats
static inline void launch_bias_grad_from_rows(const PreReduce& pre, int rows, int C, float* db) {
    const float* pp = pre(rows, C);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(C)), dim3(FIN_THREADS), 0, pre.st, pp, rows, C, db);
}
// one layer's BatchNorm fold during training: W (512, K) f32 -> out_w[512][K] T = W diag s in the layer's operand order, out_b = b + W t
template <typename T>
static inline void launch_fold_linear(const float* W, const float* b, const float* s, const float* t, void* out_w, float* out_b, int K, int mode,
                                      hipStream_t st) {
    hipLaunchKernelGGL((fold_linear_kernel<T>), dim3(512), dim3(256), 0, st, W, b, s, t, (T*)out_w, out_b, 512, K, mode);
}

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

// what a launch of the conv front end reads of its call besides its ConvArgs.  The step fills it from its pass (Pass::conv()),
// cp_debug_conv from caller buffers: both reach the conv kernels through the launch functions below, with their grid arithmetic
struct ConvLaunch {
    hipStream_t st;
    int64_t N;                  // windows
    float* partials;            // partial rows
    float* slabs;               // conv2's weight-gradient slabs [S][64][192]; the REDUCE_SLICES folded ones go behind them
    float* rows2;               // PreReduce's folded rows; conv2_wgrad_finish_kernel's rows [CONV2_FINISH_ROWS][2][64]
    const float* stats1;        // BatchNorm1's table [4][64]
    const float* pre(int& nrows, int W, int direct_rows) const { return PreReduce{partials, rows2, st}(nrows, W, direct_rows); }
};

// what a launch sequence of the 512 -> 16 projection reads of its call.  The step fills it from its pass (Pass::proj()), cp_debug_proj
// from caller buffers: both reach the projection's kernels through the launch functions below (launch_proj_fwd, proj_dz_sums,
// launch_proj_wgrad_tn, launch_proj_wgrad_onepass, proj_sums_from_wgrad; launch_proj_dgrad in gemm_ws.cuh), with their splits and grids
struct ProjLaunch {
    hipStream_t st;
    int64_t N;                  // rows
    float* partials;            // partial rows
};
// the dropout in front of the projection as set_dropout fills it; dp_thresh == 0: none
struct ProjDrop {
    uint32_t dp_thresh, dp_key;
    float dp_inv_keep;
    const uint32_t* dp_salt;
};

// where the nine statistics tables [4][C] lie: the step's workspace (Pass::stats_tables()), or cp_debug_bn's caller buffers
struct StatsTables { float* t[CP_N_BN]; };

// ---------------------------------------------------------------------------------------
// one pass: what every function of the encoder's forward and backward pass reads of its call
// ---------------------------------------------------------------------------------------
struct Pass {
    const cp_config* cfg;
    unsigned char* base;
    const WS& w;
    hipStream_t st;
    float *partials, *slabs, *coef;
    Pass(const cp_config* c, unsigned char* b, const WS& ws, hipStream_t s)
        : cfg(c), base(b), w(ws), st(s), partials((float*)(b + ws.partials)), slabs((float*)(b + ws.slabs)), coef((float*)(b + ws.coef)) {}
    int64_t N() const { return cfg->n_windows; }
    bool drop() const { return cfg->training && cfg->dp_emg > 0.f; }
    template <typename T> T* act(int l) const { return (T*)(base + w.act[l]); }
    uint8_t* act8(int l) const { return base + w.act8[l]; }
    float* stats(int l) const { return (float*)(base + w.stats[l]); }
    const float* scale(int l) const { return stats(l) + 2 * kLayerC[l]; }
    const float* shift(int l) const { return stats(l) + 3 * kLayerC[l]; }
    float* rows2() const { return (float*)(base + w.partials2); }
    PreReduce prered() const { return PreReduce{partials, rows2(), st}; }
    const float* pre(int& nrows, int W, int direct_rows = FIN_DIRECT_ROWS) const { return prered()(nrows, W, direct_rows); }
    StatsTables stats_tables() const { StatsTables s{}; for (int l = 0; l < CP_N_BN; ++l) s.t[l] = stats(l); return s; }
    ConvLaunch conv() const { return ConvLaunch{st, N(), partials, slabs, rows2(), stats(0)}; }
    ProjLaunch proj() const { return ProjLaunch{st, N(), partials}; }
};

// the dropout in front of `layer`'s consumer: threshold, key, 1 / (1 - p) and the graph-replay salt, for every argument struct that
// carries them (GemmNTArgs, ProjDrop, Proj8Args, SmFwdArgs, SmBwdArgs)
template <typename Args>
static inline void set_dropout(Args& a, const Pass& ctx, int layer) {
    a.dp_thresh = dp_thresh(ctx.cfg->dp_emg); a.dp_key = dp_key(ctx.cfg, layer); a.dp_inv_keep = dp_inv_keep(ctx.cfg->dp_emg); a.dp_salt = dp_salt(ctx.cfg);
}

// the dtype ladder of the entry points: f(TypeTag<float>) for CP_F32, f(TypeTag<bf16_t>) for 16-bit storage (CP_BF16, and what CP_FP8
// keeps in 16 bits)
template <typename T> struct TypeTag { using type = T; };
template <typename F>
static inline int by_dtype(int dtype, F f) { return dtype == CP_F32 ? f(TypeTag<float>{}) : f(TypeTag<bf16_t>{}); }

// ---------------------------------------------------------------------------------------
// encoder forward: the pieces the three forms share
// ---------------------------------------------------------------------------------------
// which statistics a forward pass normalises with, and whether it updates the running ones
struct FwdBN {
    const cp_params* p;
    const cp_bn_buffers* bn;
    bool batch_stats, have_running;
    int upd;
    float* mean(int l) const { return have_running ? bn->running_mean[l] : nullptr; }
    float* var(int l) const { return have_running ? bn->running_var[l] : nullptr; }
};
static FwdBN fwd_bn(const cp_config* c, const cp_params* p, const cp_bn_buffers* bn) {
    const bool have_running = bn && bn->running_mean[0] && bn->running_var[0];
    return FwdBN{p, bn, c->training || c->adabn, have_running, (c->training && !c->adabn && have_running) ? 1 : 0};
}

// partial rows of column sums -> layer l's statistics table.  unscale (CP_FP8): the exponent that takes the sums into true units
static int bn_finalize(const Pass& ctx, const FwdBN& f, int l, int nrows, double count, const int* unscale = nullptr) {
    if (!f.batch_stats) return 0;                       // evaluation with running statistics: all nine tables were written up front
    const cp_config* c = ctx.cfg;
    ProfScope ps(CP_K_BN_FINALIZE, ctx.st);
    const int C = kLayerC[l];
    const float* pp = ctx.pre(nrows, 2 * C);
    if (c->stats_allreduce) {          // synchronised BatchNorm: statistics of the GLOBAL batch; the row crosses the ranks in true units
        if (int e = sync_row(c, pp, nrows, 2 * C, ctx.base, ctx.w, ctx.st, &pp, nullptr, unscale)) return e;
        nrows = 1;
        count *= c->stats_world;
        unscale = nullptr;
    }
    launch_bn_finalize(pp, nrows, count, f.p->bn_g[l], f.p->bn_b[l], f.mean(l), f.var(l), f.upd, c->bn_momentum, c->bn_eps, ctx.stats(l), C, unscale, ctx.st);
    CKL("bn_finalize_kernel");
    return 0;
}

// evaluation with the running statistics: one launch writes all nine statistics tables (the caller checks the launch)
static void launch_running_stats(const cp_params* p, const cp_bn_buffers* bn, const StatsTables& stats, float eps, hipStream_t st) {
    BnRunningAll ra{};
    for (int l = 0; l < CP_N_BN; ++l) {
        ra.gamma[l] = p->bn_g[l]; ra.beta[l] = p->bn_b[l]; ra.mean[l] = bn->running_mean[l]; ra.var[l] = bn->running_var[l];
        ra.stats[l] = stats.t[l]; ra.C[l] = kLayerC[l];
    }
    ra.eps = eps;
    hipLaunchKernelGGL(bn_running_stats_kernel, dim3(CP_N_BN), dim3(512), 0, st, ra);
}
static void launch_running_stats(const Pass& ctx, const FwdBN& f) {
    launch_running_stats(f.p, f.bn, ctx.stats_tables(), ctx.cfg->bn_eps, ctx.st);
}
// ... so every BatchNorm fold of an evaluation pass (fc1..fc7 and the projection) can be made up front, in one launch instead of eight
// between the GEMMs (the caller checks the launch)
template <typename T>
static void launch_eval_folds(const cp_params* p, const StatsTables& stats, const PrepImages& im, hipStream_t st) {
    FoldBnBatch fb{};
    for (int i = 0; i < CP_N_FC; ++i) {
        const int Lp = 1 + i;
        fb.job[i] = FoldBnJob{p->fc_w[i], p->fc_b[i], stats.t[Lp] + 2 * kLayerC[Lp], stats.t[Lp] + 3 * kLayerC[Lp], im.wfc[i], im.bfc[i], 512, fcK(i),
                              i == 0 ? 1 : 0, 512};
    }
    fb.job[CP_N_FC] = FoldBnJob{p->last_w, nullptr, stats.t[8] + 2 * kLayerC[8], stats.t[8] + 3 * kLayerC[8], im.wlast, im.blast, CP_D_E, 512, 0, 32};
    hipLaunchKernelGGL((fold_linear_batch_kernel<T>), dim3(512, CP_N_FC + 1), dim3(256), 0, st, fb);
}
// the weights of the layers behind a dropout (fc5..fc7, projection) carry no BatchNorm fold: plain copies, all in one launch (the
// caller checks the launch)
template <typename T>
static void launch_fold_copies(const cp_params* p, const PrepImages& im, hipStream_t st) {
    FoldBatch fb{};
    for (int q = 0; q < 3; ++q) fb.job[q] = FoldJob{p->fc_w[4 + q], p->fc_b[4 + q], im.wfc[4 + q], im.bfc[4 + q], 512, 512, 512};
    fb.job[3] = FoldJob{p->last_w, nullptr, im.wlast, im.blast, CP_D_E, 512, 32};
    hipLaunchKernelGGL((fold_copy_batch_kernel<T>), dim3(512, 4), dim3(256), 0, st, fb);
}

// conv2's weights in the compute dtype, in the forward's and the data gradient's layout (the caller checks the launch)
template <typename T>
static inline void launch_prep_conv2(const float* conv2_w, T* fwd, T* dgr, hipStream_t st) {
    hipLaunchKernelGGL((prep_conv2_kernel<T>), dim3(48), dim3(256), 0, st, conv2_w, fwd, dgr);
}

// conv1, statistics only: r1 is never stored, its consumers recompute it from x (conv_kernels.cuh).  *rows = partial rows written;
// acc (small-batch form): the fixed-point totals of BatchNorm1
template <typename T>
static int launch_conv1_stats(const ConvLaunch& ctx, const cp_params* p, const float* x, long long* acc, const char* what, int* rows) {
    constexpr int RPP = 256 / (64 / DT<T>::EPC);                      // windows per block and pass
    const int64_t need = (ctx.N + RPP - 1) / RPP, passes = (need + 2047) / 2048;          // (caps 1024 / 512 measured: 23.6 / 23.8 us against 20.6)
    const int g = (int)((need + passes - 1) / passes);            // every block makes the same number of passes
    ProfScope ps(CP_K_CONV1_FWD, ctx.st);
    hipLaunchKernelGGL((conv1_stats_kernel<T>), dim3(g), dim3(256), 0, ctx.st, x, p->conv1_w, p->conv1_b, ctx.partials, ctx.N * 12, acc);
    CKL(what);
    *rows = g;
    return 0;
}

// conv2's forward launch: conv1 recomputed from x, BatchNorm1, conv2.  The caller adds where BatchNorm1 comes from (stats1 or bn1)
// and where the output goes (out, or out8 with its scale); *rows = partial rows written
static ConvArgs conv2_fwd_args(const Pass& ctx, const cp_params* p, const float* x, bool sums) {
    ConvArgs ca{};
    ca.x = x; ca.w1 = p->conv1_w; ca.b1 = p->conv1_b;
    ca.wc = ctx.base + ctx.w.wc2_f; ca.bias2 = p->conv2_b; ca.partials = sums ? ctx.partials : nullptr; ca.n_windows = ctx.N();
    return ca;
}
template <typename T>
static int launch_conv2_fwd(const ConvLaunch& ctx, const ConvArgs& ca, const char* what, int* rows) {
    const int g = conv_grid<T>(ctx.N);
    ProfScope ps(CP_K_CONV2_FWD, ctx.st);
    hipLaunchKernelGGL((conv2_strip_kernel<T, 0>), dim3(g), dim3(256), 0, ctx.st, ca);
    CKL(what);
    *rows = g;
    return 0;
}

// the projection's forward launch, 512 -> 16 on weights padded to 32 rows: z[N][16] f32 = A wlast^T + blast.  With a dropout
// (dp.dp_thresh != 0) the operand is dropout(scale A + shift), formed from the saved activation while staging; a_exp (bf16 kernels
// only): A holds e4m3 bytes with the scale 2^*a_exp
template <typename T>
static int launch_proj_fwd(const ProjLaunch& ctx, const void* A, const int* a_exp, const void* wlast, const float* blast,
                           const float* scale, const float* shift, const ProjDrop& dp, float* z) {
    GemmNTArgs a{};
    a.A = A; a.lda = 512; a.M = ctx.N; a.K = 512;
    a.W = wlast; a.F = 32;
    a.C = z; a.ldc = CP_D_E; a.f_valid = CP_D_E; a.bias = blast;
    a.a_exp = a_exp;
    const bool drop = dp.dp_thresh != 0;
    if (drop) {
        a.a_scale = scale; a.a_shift = shift;
        a.dp_thresh = dp.dp_thresh; a.dp_key = dp.dp_key; a.dp_inv_keep = dp.dp_inv_keep; a.dp_salt = dp.dp_salt;
    }
    if constexpr (sizeof(T) == 2) {
        if (a_exp) {
            if (drop) CK((launch_gemm_nt<T, 128, 32, ALOAD_BNDROP_F8, EPI_PLAIN_F32>(a, ctx.st)));
            else CK((launch_gemm_nt<T, 128, 32, ALOAD_F8, EPI_PLAIN_F32>(a, ctx.st)));
            return 0;
        }
    }
    if (drop) CK((launch_gemm_nt<T, 128, 32, ALOAD_BNDROP, EPI_PLAIN_F32>(a, ctx.st)));
    else CK((launch_gemm_nt<T, 128, 32, ALOAD_PLAIN, EPI_PLAIN_F32>(a, ctx.st)));
    return 0;
}

template <typename T>
static int encoder_forward_t(const cp_config* c, const cp_params* p, const cp_bn_buffers* bn, const float* x,
                             unsigned char* base, const WS& w, float* z, hipStream_t st) {
    using D = DT<T>;
    const Pass ctx(c, base, w, st);
    const int64_t N = c->n_windows, R12 = N * 12;
    const FwdBN f = fwd_bn(c, p, bn);
    const bool batch_stats = f.batch_stats, drop = ctx.drop();
    if (!batch_stats && !f.have_running) return fail(CP_ERR_ARG, "eval with stock BN needs running statistics");
    float* partials = ctx.partials;
    {
        ProfScope ps(CP_K_PREP, st);
        launch_prep_conv2<T>(p->conv2_w, (T*)(base + w.wc2_f), (T*)(base + w.wc2_d), st);
        CKL("prep_conv2_kernel");
        if (!batch_stats) {
            launch_running_stats(ctx, f);
            CKL("bn_running_stats_kernel");
            launch_eval_folds<T>(p, ctx.stats_tables(), prep_images(base, w), st);
            CKL("fold_linear_batch_kernel");
        }
        if (drop) {
            launch_fold_copies<T>(p, prep_images(base, w), st);
            CKL("fold_copy_batch_kernel");
        }
    }
    // conv1 (evaluation with running statistics needs nothing of it but its recomputation)
    if (batch_stats) {
        int g = 0;
        if (int e = launch_conv1_stats<T>(ctx.conv(), p, x, nullptr, "conv1_stats_kernel", &g)) return e;
        if (int e = bn_finalize(ctx, f, 0, g, (double)R12)) return e;
    }
    // conv2
    {
        ConvArgs ca = conv2_fwd_args(ctx, p, x, batch_stats);
        ca.stats1 = ctx.stats(0); ca.out = ctx.act<T>(1);
        int g = 0;
        if (int e = launch_conv2_fwd<T>(ctx.conv(), ca, "conv2_strip_kernel<fwd>", &g)) return e;
        if (int e = bn_finalize(ctx, f, 1, g, (double)R12)) return e;
    }
    // fc1..fc7
    for (int i = 0; i < CP_N_FC; ++i) {
        const int L = 2 + i, Lp = L - 1, K = fcK(i);
        const bool in_drop = drop && Lp >= 5;
        const T* A = ctx.act<T>(Lp);
        if (in_drop) {
            T* u = (T*)(base + w.u[Lp - 5]);
            ProfScope ps(CP_K_DROPOUT, st);
            launch_bn_dropout_apply<T>(ctx.act<T>(Lp), ctx.stats(Lp), u, N, dp_thresh(c->dp_emg), dp_key(c, Lp), dp_inv_keep(c->dp_emg), dp_salt(c), st);
            CKL("bn_dropout_apply_kernel");
            A = u;
        }
        if (!in_drop && batch_stats) {          // (the layers behind a dropout were copied by fold_copy_batch_kernel above; running statistics: folded up front)
            ProfScope ps(CP_K_FOLD, st);
            launch_fold_linear<T>(p->fc_w[i], p->fc_b[i], ctx.scale(Lp), ctx.shift(Lp), base + w.wfc[i], (float*)(base + w.bfc[i]), K, i == 0 ? 1 : 0, st);
            CKL("fold_linear_kernel");
        }
        GemmNTArgs a{};
        a.A = A; a.lda = K; a.M = N; a.K = K;
        a.W = base + w.wfc[i]; a.F = 512;
        a.C = ctx.act<T>(L); a.ldc = 512; a.bias = (float*)(base + w.bfc[i]); a.relu = 1;
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
        if (int e = bn_finalize(ctx, f, L, nrows, (double)N)) return e;
    }
    // projection 512 -> 16 (weights padded to 32 rows)
    {
        const int Lp = 8;
        // dropout(BN(fc7)) is NOT written out for the projection: its two consumers (this launch and the projection's weight
        // gradient) form it from the saved activation while staging their operand -- both are bound by reading those 172 MB, and
        // the pass that materialised it moved 344 MB.  (That pass, as fc4..fc6 keep it, was removed here; see git history.)
        if (!drop && batch_stats) {        // (with dropout: copied by fold_copy_batch_kernel at the start of the pass; running statistics: folded up front)
            ProfScope ps(CP_K_FOLD, st);
            launch_proj_fold<T>(p->last_w, ctx.scale(Lp), ctx.shift(Lp), base + w.wlast, (float*)(base + w.blast), st);
            CKL("fold_linear_kernel(last)");
        }
        ProjDrop dp{};
        if (drop) set_dropout(dp, ctx, Lp);
        ProfScope ps(CP_K_PROJ_FWD, st);
        if (int e = launch_proj_fwd<T>(ctx.proj(), ctx.act<T>(Lp), nullptr, base + w.wlast, (float*)(base + w.blast), ctx.scale(Lp), ctx.shift(Lp), dp, z)) return e;
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
    const Pass ctx(c, base, w, st);
    const int64_t N = c->n_windows, R12 = N * 12;
    const FwdBN f = fwd_bn(c, p, bn);
    const bool batch_stats = f.batch_stats, drop = ctx.drop();
    if (!batch_stats && !f.have_running) return fail(CP_ERR_ARG, "eval with stock BN needs running statistics");
    // (cp_config.tile_schedule is not consulted: the 8-bit kernels are weight-stationary, i.e. statically scheduled; a packed sweep
    //  that asks for the dynamic schedule gets it on its 16/32-bit configurations)
    float* partials = ctx.partials;
    Fp8State* fs = (Fp8State*)(base + w.f8state);
    {
        ProfScope ps(CP_K_PREP, st);
        hipLaunchKernelGGL(fp8_update_scales_kernel, dim3(1), dim3(64), 0, st, fs, N);
        launch_prep_conv2<T>(p->conv2_w, (T*)(base + w.wc2_f), (T*)(base + w.wc2_d), st);
        if (!batch_stats) launch_running_stats(ctx, f);
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
    if (batch_stats) {
        int g = 0;
        if (int e = launch_conv1_stats<T>(ctx.conv(), p, x, nullptr, "conv1_stats_kernel", &g)) return e;
        if (int e = bn_finalize(ctx, f, 0, g, (double)R12)) return e;
    }
    {
        ConvArgs ca = conv2_fwd_args(ctx, p, x, batch_stats);
        ca.stats1 = ctx.stats(0);
        ca.out8 = ctx.act8(1); ca.out_exp = &fs->e[F8_T_ACT + 1]; ca.out_amax = &fs->amax[F8_T_ACT + 1];
        int g = 0;
        if (int e = launch_conv2_fwd<T>(ctx.conv(), ca, "conv2_strip_kernel<fwd, e4m3>", &g)) return e;
        if (int e = bn_finalize(ctx, f, 1, g, (double)R12)) return e;      // (its sums are of the bf16-rounded values in true units)
    }
    if (!batch_stats) {
        // evaluation with the running statistics (no dropout): statistics and scale table are final, so the seven folds are one launch
        ProfScope ps(CP_K_FOLD, st);
        Fold8Batch fb{};
        for (int i = 0; i < CP_N_FC; ++i) {
            const int Lp = 1 + i;
            fb.job[i] = Fold8Job{p->fc_w[i], p->fc_b[i], ctx.scale(Lp), ctx.shift(Lp), base + w.wfc8[i], base + w.wsc8[i],
                                 (float*)(base + w.bfc[i]), fcK(i), i == 0 ? 1 : 0, F8_T_ACT + Lp, F8_T_ACT + 2 + i};
        }
        hipLaunchKernelGGL(fold_linear8_batch_kernel, dim3(512, CP_N_FC), dim3(256), 0, st, fb, (const Fp8State*)fs);
        CKL("fold_linear8_batch_kernel");
    }
    // fc1..fc7
    for (int i = 0; i < CP_N_FC; ++i) {
        const int L = 2 + i, Lp = L - 1, K = fcK(i);
        const bool in_drop = drop && Lp >= 5;
        const uint8_t* A = ctx.act8(Lp);
        int t_in = F8_T_ACT + Lp;
        if (in_drop) {
            uint8_t* u = base + w.u8[Lp - 5];
            t_in = F8_T_U + (Lp - 5);
            ProfScope ps(CP_K_DROPOUT, st);
            launch_bn_dropout_apply8(A, ctx.stats(Lp), u, N, dp_thresh(c->dp_emg), dp_key(c, Lp), dp_inv_keep(c->dp_emg), dp_salt(c), fs, F8_T_ACT + Lp,
                                     t_in, st);
            CKL("bn_dropout_apply8_kernel");
            A = u;
        }
        if (batch_stats && !in_drop) {     // (running statistics: all seven folds were made in one launch before the loop; behind a dropout: in the prep launch)
            ProfScope ps(CP_K_FOLD, st);
            launch_fold_linear8(p->fc_w[i], p->fc_b[i], ctx.scale(Lp), ctx.shift(Lp), base + w.wfc8[i], base + w.wsc8[i], (float*)(base + w.bfc[i]), K,
                                i == 0 ? 1 : 0, fs, t_in, F8_T_ACT + L, st);
            CKL("fold_linear8_kernel");
        }
        Ws8Args a{};
        a.A = A; a.W = base + w.wfc8[i]; a.wsc = base + w.wsc8[i]; a.bias = (float*)(base + w.bfc[i]);
        a.C = ctx.act8(L); a.partials = batch_stats ? partials : nullptr; a.amax = &fs->amax[F8_T_ACT + L]; a.M = N; a.F = 512;     // (nullptr: no column sums)
        int nrows = 0;
        {
            ProfScope ps(K == 512 ? CP_K_FC_FWD_WS : CP_K_FC_FWD, st);
            if (K == 512) CK(launch_gemm_ws8<512>(a, st, &nrows));
            else CK(launch_gemm_ws8<768>(a, st, &nrows));
        }
        if (int e = bn_finalize(ctx, f, L, nrows, (double)N, &fs->e[F8_T_ACT + L])) return e;
    }
    // projection 512 -> 16 on the bf16 kernel: its operand is read as e4m3 and converted (and, with dropout, turned into
    // dropout(BN(fc7))) while staging
    {
        const int Lp = 8;
        {
            ProfScope ps(CP_K_FOLD, st);
            launch_proj_fold<T>(p->last_w, drop ? (const float*)nullptr : ctx.scale(Lp), drop ? (const float*)nullptr : ctx.shift(Lp), base + w.wlast,
                                (float*)(base + w.blast), st);
            CKL("fold_linear_kernel(last)");
        }
        ProjDrop dp{};
        if (drop) set_dropout(dp, ctx, Lp);
        ProfScope ps(CP_K_PROJ_FWD, st);
        if (int e = launch_proj_fwd<T>(ctx.proj(), ctx.act8(Lp), &fs->e[F8_T_ACT + Lp], base + w.wlast, (float*)(base + w.blast), ctx.scale(Lp), ctx.shift(Lp), dp, z)) return e;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// small batches (csrc/small.cuh): N <= 64 groups, batch statistics, f32 or bf16
// ---------------------------------------------------------------------------------------
static bool use_small(const cp_config* c) {
    return c->n_windows <= SM_MAX_WINDOWS && (c->training || c->adabn) && c->dtype != CP_FP8 && !c->stats_allreduce && !opt(c, CP_OPT_NO_SMALL);
}

template <typename T>
static int encoder_forward_small_t(const cp_config* c, const cp_params* p, const cp_bn_buffers* bn, const float* x,
                                   unsigned char* base, const WS& w, float* z, hipStream_t st) {
    const Pass ctx(c, base, w, st);
    const int64_t N = c->n_windows, R12 = N * 12;
    const FwdBN f = fwd_bn(c, p, bn);
    const bool drop = ctx.drop();
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
        b.gamma = p->bn_g[l]; b.beta = p->bn_b[l]; b.stats = ctx.stats(l);
        b.running_mean = f.mean(l); b.running_var = f.var(l);
        b.update_running = f.upd; b.momentum = c->bn_momentum; b.eps = c->bn_eps;
        return b;
    };
    int g = 0;
    if (int e = launch_conv1_stats<T>(ctx.conv(), p, x, acc_of(0), "conv1 (small)", &g)) return e;
    {
        ConvArgs ca = conv2_fwd_args(ctx, p, x, true);
        ca.bn1 = bn_of(0); ca.acc_out = acc_of(1); ca.out = ctx.act<T>(1);
        if (int e = launch_conv2_fwd<T>(ctx.conv(), ca, "conv2 (small)", &g)) return e;
    }
    // fc1..fc7 and the projection: each launch turns its input's two fixed-point totals per column into scale / shift itself
    for (int i = 0; i < CP_N_FC; ++i) {
        const int L = 2 + i, Lp = L - 1, K = fcK(i);
        SmFwdArgs a{};
        a.A = ctx.act<T>(Lp); a.W = base + w.wfc[i]; a.bias = p->fc_b[i]; a.C = ctx.act<T>(L); a.out_acc = acc_of(L);
        a.bn_in = bn_of(Lp); a.smod = kLayerC[Lp]; a.N = N; a.K = K;
        if (drop && Lp >= 5) set_dropout(a, ctx, Lp);
        ProfScope ps(K == 512 ? CP_K_FC_FWD_WS : CP_K_FC_FWD, st);
        if (ks) hipLaunchKernelGGL((sm_fc_fwd_kernel<T, 0, true>), dim3(tiles_m * (512 / SmTile<true>::BN)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sm_fc_fwd_kernel<T, 0>), dim3(tiles_m * (512 / SM_BN)), dim3(256), 0, st, a);
        CKL("sm_fc_fwd_kernel");
    }
    {
        SmFwdArgs a{};
        a.A = ctx.act<T>(8); a.W = base + w.wlast; a.C = z; a.bn_in = bn_of(8); a.smod = 512; a.N = N; a.K = 512;
        if (drop) set_dropout(a, ctx, 8);
        ProfScope ps(CP_K_PROJ_FWD, st);
        hipLaunchKernelGGL((sm_fc_fwd_kernel<T, 1>), dim3(tiles_m), dim3(256), 0, st, a);
        CKL("sm_fc_fwd_kernel<proj>");
    }
    return 0;
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
    unsigned char* base = (unsigned char*)ws;
    const hipStream_t st = (hipStream_t)stream;
    // second stream (cp_config.aux_stream): the transposed weights of the backward pass are made beside the forward pass -- bf16 from its
    // start, CP_FP8 behind it (their scale bytes need this step's gradient exponents, set by the forward's first launch)
    const int path = forward_path(cfg);
    const bool drop = cfg->training && cfg->dp_emg > 0.f;
    const Aux aux = make_aux(cfg, st, drop && path != PATH_SMALL && cfg->dtype != CP_F32 && !dyn_tiles(cfg) &&
                                          !opt(cfg, CP_OPT_UNPAIRED_WGRAD) && !opt(cfg, CP_OPT_UNFUSED_BN_BWD) && !opt(cfg, CP_OPT_FP8_BRIDGE));
    if (cp_forward_record* r = cfg->record)
        *r = cp_forward_record{cfg->n_windows, path, 0, aux.on ? 1 : 0, 0, aux.on ? (void*)aux.join_ev : nullptr};
    if (path == PATH_FP8) {
        if (int e = encoder_forward_fp8(cfg, p, bn, x, base, w, z_out, st)) return e;
    }
    if (aux.on) {
        if (int e = aux.fork()) return e;
        if (int e = path == PATH_FP8 ? launch_weight_transposes_fp8(p, base, w, aux.side) : launch_weight_transposes<bf16_t>(p, base, w, aux.side)) return e;
        CK(hipEventRecord(aux.join_ev, aux.side));          // (waited for by cp_encoder_backward)
    }
    if (path == PATH_FP8) return 0;
    return by_dtype(cfg->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return path == PATH_SMALL ? encoder_forward_small_t<T>(cfg, p, bn, x, base, w, z_out, st) : encoder_forward_t<T>(cfg, p, bn, x, base, w, z_out, st);
    });
}

// ---------------------------------------------------------------------------------------
// encoder backward: the pieces the forms share
// ---------------------------------------------------------------------------------------
// test aid (cp_config.grad_tap): device buffer of 9 slots x n_windows x 768 elements of the compute dtype (CP_FP8: bf16) that receives a
// copy of every intermediate gradient of the backward pass, so that each backward kernel can be checked on its own
// inputs at full batch size (tests/test_gpu_fullsize.py).  nullptr (the default) = no copies.  A tap never changes which kernels compute
// the step: it adds copies and one stand-alone conv2 data-gradient launch for slot 0 (conv_backward_tail), and keeps the second stream
// off (make_aux).
// The small-batch form fills 11 slots (tests/test_gpu_small_recompute.py; the slots' meaning on that path: include/cpnative.h).
// check_tap(): the whole buffer is checked once, before the first launch of a backward pass -- a short one enqueues nothing.
static int check_tap(const cp_config* c, bool small) {
    if (!c->grad_tap) return 0;
    const size_t slot_bytes = (size_t)c->n_windows * 768 * (c->dtype == CP_F32 ? 4 : 2);
    if ((size_t)(small ? 11 : 9) * slot_bytes > c->grad_tap_bytes) return fail(CP_ERR_ARG, "gradient tap buffer too small");
    return 0;
}
static int tap_gradient(const cp_config* c, int slot, const void* src, int64_t n_windows, int width, size_t es, hipStream_t st) {
    if (!c->grad_tap) return 0;
    const size_t slot_bytes = (size_t)n_windows * 768 * es, bytes = (size_t)n_windows * width * es;
    CK(hipMemcpyAsync((unsigned char*)c->grad_tap + slot * slot_bytes, src, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

// rows per split of a weight-gradient launch, rounded up to `round` rows (and at least that many where `floor_rows`)
static inline void split_rows(int64_t M, int target_splits, int* splits, int64_t* rows_per_split, int round = 32, bool floor_rows = true) {
    int64_t rps = (M + target_splits - 1) / target_splits;
    rps = ((rps + round - 1) / round) * round;
    if (floor_rows && rps < round) rps = round;
    *rows_per_split = rps;
    *splits = (int)((M + rps - 1) / rps);
}
// the row split of an 8-bit weight-gradient launch (gemm_tn8_kernel: 64-row stages, rows past the end zero-filled): 64 splits for a
// 512 x 512 layer, 40 for fc1's 512 x 768, 32 per problem of a paired launch
static inline void split_rows_tn8(int64_t M, bool paired, int Q, int* splits, int64_t* rows_per_split) {
    split_rows(M, paired ? 32 : (Q == 512 ? 64 : 40), splits, rows_per_split, 64, false);
}
// the fold of its bf16 slabs: the two tensors' scale exponents (device words of the scale table) are divided out
static inline void launch_reduce_slabs8(const float* slabs, int S, int Q, const float* s, const float* t, const float* dbsum, float* grad, int mode,
                                        float* raw, const int* exp_x, const int* exp_y, hipStream_t st) {
    hipLaunchKernelGGL(reduce_slabs_kernel<bf16_t>, dim3(512), dim3(256), 0, st, slabs, S, 512, Q, 512, s, t, dbsum, grad, mode, raw, exp_x, exp_y);
}

// BatchNorm backward, step 1 for layer l (C channels, each seen nfold times in the partial rows): sums -> coefficients of
// the data gradient + dgamma / dbeta.  Synchronised BatchNorm: the coefficients take the sums and the count of ALL ranks,
// dgamma / dbeta this rank's own sums (the gradient all-reduce adds the ranks' parts).
static int bwd_finalize(const Pass& ctx, cp_params* g, const float* pp, int nr, double count, int l, int C, int nfold, const char* what) {
    const cp_config* c = ctx.cfg;
    const float* local = nullptr;
    if (c->stats_allreduce) {
        if (int e = sync_row(c, pp, nr, 2 * C * nfold, ctx.base, ctx.w, ctx.st, &pp, &local)) return e;
        nr = 1;
        count *= c->stats_world;
    }
    launch_bn_bwd_finalize(pp, nr, count, ctx.stats(l), ctx.coef, g->bn_g[l], g->bn_b[l], C, nfold, local, ctx.st);
    CKL(what);
    return 0;
}

// BatchNorm backward, step 1 without a launch: a persistent consumer (gemm_wsd16_kernel<0>, proj_dgrad_kernel, conv2_dgrad_conv1_kernel) folds
// the `nr` partial rows in its prologue, every block for its own channels, with bn_bwd_finalize_kernel's order of additions and
// expressions (common.cuh, bnp_*).  Not under synchronised BatchNorm (a row crosses the ranks between the two launches), not with
// more rows than the kernel's prologue walks, not under CP_OPT_FINALIZE_LAUNCHES.  The rows must not lie in the buffer the consumer
// writes its own partial rows to (a block that starts late reads them while an early one finishes): the producers write to ctx.rows2().
static inline bool bwd_in_prologue(const Pass& ctx, int nr, int max_rows) {
    return !opt(ctx.cfg, CP_OPT_FINALIZE_LAUNCHES) && !ctx.cfg->stats_allreduce && nr <= max_rows;
}
static inline void set_bn_prologue(GemmNTArgs& a, const Pass& ctx, cp_params* g, const float* rows, int nr, double count, int l) {
    a.bn_rows = rows; a.bn_nr = nr; a.bn_stats = ctx.stats(l); a.bn_count = count; a.bn_dgamma = g->bn_g[l]; a.bn_dbeta = g->bn_b[l];
}

// a bias gradient = the column sums of `rows` partial rows of C floats (ctx.partials)
static int bias_grad_from_rows(const Pass& ctx, int rows, int C, float* db, const char* what) {
    launch_bias_grad_from_rows(ctx.prered(), rows, C, db);
    CKL(what);
    return 0;
}

// projection without a dropout in front: the column sums of dz, and from them and the RAW weight-gradient product (praw) the
// BatchNorm-backward sums of fc7's BatchNorm in one partial row -- no N-sized read
template <typename T>
static int proj_dz_sums(const ProjLaunch& ctx, const T* dz, float* dzsum) {
    using D = DT<T>;
    const int gb = grid_rows(ctx.N, 256 / (CP_D_E / D::EPC), 64);
    hipLaunchKernelGGL((colsum_kernel<T>), dim3(gb), dim3(256), 256 * D::EPC * 4, ctx.st, dz, ctx.partials, ctx.N, 64, CP_D_E);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(FIN_GRID(CP_D_E)), dim3(FIN_THREADS), 0, ctx.st, ctx.partials, gb, CP_D_E, dzsum);  // 16 columns: tiny
    CKL("colsum(dz)");
    return 0;
}
static int proj_sums_from_wgrad(const ProjLaunch& ctx, const float* Wp, const float* praw, const float* dzsum) {
    hipLaunchKernelGGL(bn_bwd_sums_from_wgrad_kernel, dim3(512 / 64, 1), dim3(256), 0, ctx.st, praw, Wp, dzsum, ctx.partials, CP_D_E, 512, 0);
    CKL("bn_bwd_sums_from_wgrad_kernel(last)");
    return 0;
}

// the projection's weight gradient as two launches on stream sw: gemm_tn_kernel<T, 64, 128, .> over kProjSplits row splits ->
// slabs[S][64][512], reduce_slabs_kernel -> dW (16, 512) = s P + t dzsum (s NULL: the plain product) and the raw product praw (or
// NULL).  Y is the saved activation [N][512] (y_exp, bf16 kernels only: as e4m3 bytes); behind a dropout (dp.dp_thresh != 0) the
// operand is dropout(y_scale Y + y_shift), formed while staging.  *splits = S
template <typename T>
static int launch_proj_wgrad_tn(const ProjLaunch& ctx, hipStream_t sw, const T* dz, const void* Y, const int* y_exp, float* slabs,
                                const float* y_scale, const float* y_shift, const ProjDrop& dp, const float* s, const float* t,
                                const float* dzsum, float* dW, float* praw, int* splits) {
    GemmTNArgs ta{};
    ta.X = dz; ta.ldx = 64; ta.Y = Y; ta.ldy = 512; ta.slabs = slabs; ta.M = ctx.N; ta.P = 64; ta.Q = 512;
    ta.y_exp = y_exp;
    int S;
    split_rows(ctx.N, kProjSplits, &S, &ta.rows_per_split);
    if (dp.dp_thresh != 0) {
        // u8 = dropout(BN(fc7)) was never written (encoder_forward_t): formed from the saved activation while staging
        ta.y_scale = y_scale; ta.y_shift = y_shift;
        ta.dp_thresh = dp.dp_thresh; ta.dp_key = dp.dp_key; ta.dp_inv_keep = dp.dp_inv_keep; ta.dp_salt = dp.dp_salt;
        CK((launch_gemm_tn<T, 64, 128, YLOAD_BNDROP>(ta, S, sw)));
    } else if (y_exp) {
        if constexpr (sizeof(T) == 2) CK((launch_gemm_tn<T, 64, 128, YLOAD_F8>(ta, S, sw)));
        else return fail(CP_ERR_ARG, "an e4m3 operand feeds the bf16 kernels");
    } else {
        CK((launch_gemm_tn<T, 64, 128, YLOAD_PLAIN>(ta, S, sw)));
    }
    hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(32), dim3(256), 0, sw, ta.slabs, S, 64, 512, CP_D_E, s, t, dzsum, dW, 0, praw,
                       (const int*)nullptr, (const int*)nullptr);
    CKL("reduce_slabs(last)");
    *splits = S;
    return 0;
}

// the projection's weight gradient behind fc7's dropout in one pass over the saved activation R (gemm_tn.cuh): proj_wgrad_sums_kernel
// (r_exp: <true>, R as e4m3 bytes) -> slabs[S][32][512], proj_wgrad_finish_kernel -> dW (16, 512) and PROJ_FINISH_ROWS partial rows
// [2][512] of fc7's BatchNorm-backward sums in ctx.partials.  *splits = S
static int launch_proj_wgrad_onepass(const ProjLaunch& ctx, const bf16_t* dz, const void* R, const int* r_exp, float* slabs,
                                     const ProjDrop& dp, const float* scale, const float* shift, const float* Wp, float* dW, int* splits) {
    ProjWgradArgs pa{};
    pa.dz = dz; pa.R = R; pa.slabs = slabs; pa.M = ctx.N;
    int S;
    split_rows(ctx.N, kProjSplits, &S, &pa.rows_per_split);
    pa.splits = S;
    // (ProjWgradArgs has no 1 / (1 - p): proj_wgrad_finish_kernel applies it to the finished product)
    pa.dp_thresh = dp.dp_thresh; pa.dp_key = dp.dp_key; pa.dp_salt = dp.dp_salt;
    if (r_exp) {
        hipLaunchKernelGGL(proj_wgrad_sums_kernel<true>, dim3(PROJ_WGRAD_GRID(S)), dim3(256), 0, ctx.st, pa);
        CKL("proj_wgrad_sums_kernel<e4m3>");
    } else {
        hipLaunchKernelGGL(proj_wgrad_sums_kernel<false>, dim3(PROJ_WGRAD_GRID(S)), dim3(256), 0, ctx.st, pa);
        CKL("proj_wgrad_sums_kernel");
    }
    hipLaunchKernelGGL(proj_wgrad_finish_kernel, dim3(32, PROJ_FINISH_ROWS), dim3(256), 0, ctx.st, slabs, S, scale, shift, Wp, dp.dp_inv_keep, r_exp,
                       dW, ctx.partials);
    CKL("proj_wgrad_finish_kernel");
    *splits = S;
    return 0;
}

// Where fc layer i's weight gradient runs.  defer: behind a dropout the layer's BN-backward sums do not come from its weight
// gradient, so nothing needs the gradient before the optimiser -- fc7's and fc5's are deferred by one layer and run in ONE launch
// with the next layer's (the gradient buffer they read is the ping-pong partner, untouched until that layer's data gradient): two
// problems x 4 tiles x 32 splits fill the GPU with half the f32 slabs per layer (134 -> 67 MB written and re-read).
// Second stream: the weight gradients behind a dropout and their slab reductions float there (sw, slabs); fc7 waits for fc6 as
// before -- one paired launch -- but fc5 goes alone: fc4's weight gradient is on the critical path, its product carries the
// BatchNorm-backward sums of the layer below.
struct WgradPlace {
    bool defer;
    hipStream_t sw;
    float* slabs;
};
static int place_wgrad(const Pass& ctx, const Aux& aux, bool in_drop, int i, bool may_pair, WgradPlace* pl) {
    pl->defer = may_pair && in_drop && (i == 6 || (i == 4 && !aux.on)) && fcK(i - 1) == 512;
    const bool floats = aux.on && in_drop;
    pl->sw = floats ? aux.side : ctx.st;
    pl->slabs = floats ? (float*)(ctx.base + ctx.w.slabs_b) : ctx.slabs;
    if (floats && !pl->defer) return aux.fork();      // cur (and the deferred layer's gradient, and both bias gradients) are final
    return 0;
}

// the gradient buffers of the next fc layer.  Second stream: the gradients the floating launches read (layers 8, 7, 6) stay where
// they are -- keep2 and the ping-pong pair take over one by one; from layer 5 on, and on one stream, the usual ping-pong
template <typename B>
static inline void rotate_grads(B*& cur, B*& nxt, bool aux_on, int L, B* keep2, B* ping0, B* ping1) {
    if (aux_on && L >= 6) {
        cur = nxt;
        nxt = L == 8 ? keep2 : (L == 7 ? ping0 : ping1);
    } else {
        B* tmp = cur; cur = nxt; nxt = tmp;
    }
}

// conv2's weight gradient: the RAW product g^T r1 in slabs (the image holds conv1's rounded ReLU output), the slabs folded, and the
// finish launch -- BatchNorm1's scale and shift applied to the 64 x 192 result, and from the same product BatchNorm1's backward sums
// (rows2).  small: the small-batch kernel, which applies BatchNorm2 + ReLU backward while staging and leaves the bias-gradient rows in
// gcols3 (the caller has filled those fields of ca); g8: `cur` holds e5m2 bytes.  gcols / gcol_rows: the column sums of the gradient
template <typename T>
static int conv2_wgrad(const ConvLaunch& ctx, const cp_params* p, cp_params* g, ConvArgs& ca, bool small, bool g8, const float* gcols, int gcol_rows,
                       const float* gcols3, float* db2, int* nslabs = nullptr) {
    const hipStream_t st = ctx.st;
    float* slabs = ctx.slabs;
    ProfScope ps(CP_K_CONV2_WGRAD, st);
    const int64_t strips = (ctx.N + CONV_WG_WPB - 1) / CONV_WG_WPB;
    const int64_t cap = (small || sizeof(T) == 2) ? 512 : 256;      // two blocks per CU (194 registers with the strip prefetch)
    const int S = (int)(strips < cap ? strips : cap);
    ca.partials = slabs;
    if (small) {
        hipLaunchKernelGGL((conv2_wgrad_kernel<T, false, true>), dim3(S), dim3(256), 0, st, ca);
    } else if constexpr (sizeof(T) == 2) {
        if (g8) hipLaunchKernelGGL((conv2_wgrad_kernel<T, true>), dim3(S), dim3(256), 0, st, ca);
        else hipLaunchKernelGGL((conv2_wgrad_kernel<T>), dim3(S), dim3(256), 0, st, ca);
    } else {
        hipLaunchKernelGGL((conv2_wgrad_kernel<T>), dim3(S), dim3(256), 0, st, ca);
    }
    CKL(small ? "conv2_wgrad_kernel<small>" : "conv2_wgrad_kernel");
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
    hipLaunchKernelGGL((conv2_wgrad_finish_kernel<T>), dim3(CONV2_FINISH_ROWS), dim3(256), 0, st, sl, ns, gcols, small ? S : gcol_rows, p->conv2_w,
                       ctx.stats1, g->conv2_w, ctx.rows2, gcols3, db2);
    CKL(small ? "conv2_wgrad_finish_kernel<small>" : "conv2_wgrad_finish_kernel");
    if (nslabs) *nslabs = S;
    return 0;
}

// conv1's gradients from the partial rows of conv2_dgrad_conv1_kernel
static int conv1_bwd_finalize(const ConvLaunch& ctx, int rows, cp_params* g) {
    ProfScope ps(CP_K_CONV1_BWD, ctx.st);
    const float* pp = ctx.pre(rows, 4 * 64, 2 * REDUCE_SLICES);
    hipLaunchKernelGGL(conv1_bwd_finalize_kernel, dim3(1), dim3(256), 0, ctx.st, pp, rows, g->conv1_w, g->conv1_b);
    CKL("conv1_bwd_finalize_kernel");
    return 0;
}

// column sums of conv2's gradient per (position, channel), for a caller without fc1's bias-gradient rows: one pass over the tensor.
// *rows = partial rows [768] written
template <typename T>
static int launch_conv2_gcols(const ConvLaunch& ctx, const T* cur, int* rows) {
    constexpr int cpr = 768 / DT<T>::EPC, rpp = 256 / cpr;
    int64_t gb = (ctx.N + rpp - 1) / rpp;
    if (gb > 256) gb = 256;
    ProfScope ps(CP_K_BN_BWD, ctx.st);
    hipLaunchKernelGGL((colsum_kernel<T>), dim3((int)gb), dim3(256), (size_t)rpp * 768 * 4, ctx.st, cur, ctx.partials, ctx.N, 768, 768);
    CKL("colsum_kernel(conv2 gradient)");
    *rows = (int)gb;
    return 0;
}

// conv2's data gradient on its own (the gradient tap's): ca.out = dL/d(BN1 output), *rows = partial rows [2][64] written
template <typename T>
static int launch_conv2_dgrad(const ConvLaunch& ctx, const ConvArgs& ca, int* rows) {
    const int g = conv_grid<T>(ctx.N);
    hipLaunchKernelGGL((conv2_strip_kernel<T, 1>), dim3(g), dim3(256), 0, ctx.st, ca);
    CKL("conv2_strip_kernel<dgrad>");
    *rows = g;
    return 0;
}

// conv2's data gradient, BatchNorm1 + ReLU backward and conv1's gradients in one pass over the gradient: *rows = partial rows
// [4][64] written.  small: BatchNorm1's backward finalised in the prologue; g8: ca.gin holds e5m2 bytes
template <typename T>
static int launch_conv2_dgrad_conv1(const ConvLaunch& ctx, const ConvArgs& ca, bool small, bool g8, int* rows) {
    const int g = conv_grid<T>(ctx.N);
    const hipStream_t st = ctx.st;
    ProfScope ps(CP_K_CONV2_DGRAD, st);
    if (small) {
        hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T, false, true>), dim3(g), dim3(256), 0, st, ca);
    } else if constexpr (sizeof(T) == 2) {
        if (g8) hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T, true>), dim3(g), dim3(256), 0, st, ca);
        else hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T>), dim3(g), dim3(256), 0, st, ca);
    } else {
        hipLaunchKernelGGL((conv2_dgrad_conv1_kernel<T>), dim3(g), dim3(256), 0, st, ca);
    }
    CKL(small ? "conv2_dgrad_conv1_kernel<small>" : "conv2_dgrad_conv1_kernel");
    *rows = g;
    return 0;
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
    const Pass ctx(c, base, w, st);
    const int64_t N = c->n_windows, R12 = N * 12;
    float* partials = ctx.partials;
    // (round 4: conv2's weight gradient is on the critical path again -- BatchNorm1's backward sums follow from it -- so nothing of
    //  the conv stack floats on the second stream)
    // every gradient but the conv stack's is final here (cp_encoder_backward_ev): a data-parallel caller starts summing
    // them across ranks while the conv backward below still runs
    if (fc_grads_ready) {
        if (aux) { if (int e = aux->join()) return e; }          // (the fc weight gradients that ran on the second stream included)
        CK(hipEventRecord(fc_grads_ready, st));
    }
    if (small && (bn_done || g8 || c->stats_allreduce)) return fail(CP_ERR_ARG, "conv_backward_tail: small-batch form");
    // ---- conv2: cur = dL/d(BN2 output) as [N][768] == [(N*12)][64] -------------------------
    if (!small && !bn_done) {
        ProfScope ps(CP_K_BN_BWD, st);
        int nr = stat_rows;          // 1: fc1's input (conv2's BN) never has dropout
        const float* pp = ctx.pre(nr, 2 * 768);
        if (int e = bwd_finalize(ctx, g, pp, nr, (double)R12, 1, 64, 12, "bn_bwd_finalize_kernel(conv2)")) return e;
        const int gb = launch_bn_relu_bwd<T>(cur, ctx.act<T>(1), ctx.coef, partials, R12, 64, 2048, st);
        if (int e = bias_grad_from_rows(ctx, gb, 64, g->conv2_b, "bn_relu_bwd_kernel(conv2)")) return e;
        gcol_rows = 0;
    }
    if (g8) {
        if (gcol_rows <= 0 || sizeof(T) != 2) return fail(CP_ERR_ARG, "conv_backward_tail: 8-bit gradient without its column sums");
        if (c->grad_tap) {
            const size_t slot_bytes = (size_t)N * 768 * 2;
            hipLaunchKernelGGL(dequant5_bf16_kernel, dim3(1024), dim3(256), 0, st, (const uint8_t*)cur, (bf16_t*)((unsigned char*)c->grad_tap + slot_bytes),
                               N * 192, g8, F8_T_GRAD + 1);
            CKL("dequant5_bf16_kernel(conv2 gradient)");
        }
    } else if (!small) {
        if (int e = tap_gradient(c, 1, cur, N, 768, sizeof(T), st)) return e;         // dL/d(conv2 pre-activation), [w][c]
    }
    // column sums of that gradient per (position, channel): `partials` still holds them as fc1's data-gradient launch wrote them
    // (gcol_rows rows of 768, its bias-gradient rows); a caller without such rows gets them from one pass over the tensor
    if (!small && gcol_rows <= 0) {
        if (int e = launch_conv2_gcols<T>(ctx.conv(), cur, &gcol_rows)) return e;
    }
    ConvArgs ca{};
    ca.x = x; ca.w1 = p->conv1_w; ca.b1 = p->conv1_b; ca.stats1 = nullptr; ca.gin = cur; ca.n_windows = N;
    if (small) {
        // (the weight-gradient kernel finalises BatchNorm2's backward from fc1's rows and writes dL/d(conv2 pre-activation) back in place)
        float* gcols3 = (float*)(base + w.praw);
        ca.bn2_rows = partials; ca.bn2_nr = stat_rows; ca.r2 = ctx.act<T>(1); ca.stats2 = ctx.stats(1);
        ca.dgamma2 = g->bn_g[1]; ca.dbeta2 = g->bn_b[1]; ca.gcols3 = gcols3;
        if (int e = conv2_wgrad<T>(ctx.conv(), p, g, ca, true, false, nullptr, 0, gcols3, g->conv2_b)) return e;
        if (int e = tap_gradient(c, 1, cur, N, 768, sizeof(T), st)) return e;
    } else {
        ca.gin_exp = g8 ? (const int*)&g8->e[F8_T_GRAD + 1] : nullptr;
        if (int e = conv2_wgrad<T>(ctx.conv(), p, g, ca, false, g8 != nullptr, partials, gcol_rows, nullptr, nullptr)) return e;
        ProfScope ps(CP_K_BN_BWD, st);          // (the profiler keeps its record of this step of the plan; with the prologue it brackets no launch)
        if (!g8 && bwd_in_prologue(ctx, CONV2_FINISH_ROWS, BNP_MAX_ROWS)) {
            // BatchNorm1's backward is finalised in conv2_dgrad_conv1_kernel's prologue, from the finish launch's rows and with the finalize
            // launch's bits (the 8-bit step keeps the launch)
            ca.stats1 = ctx.stats(0); ca.rows1 = ctx.rows2(); ca.rows1_nr = CONV2_FINISH_ROWS;
            ca.dgamma1 = g->bn_g[0]; ca.dbeta1 = g->bn_b[0];
        } else {
            if (int e = bwd_finalize(ctx, g, ctx.rows2(), CONV2_FINISH_ROWS, (double)R12, 0, 64, 1, "bn_bwd_finalize_kernel(conv1)")) return e;
            ca.coef = ctx.coef;
        }
    }
    int grid_d = 0;
    ca.wc = base + w.wc2_d;
    if (c->grad_tap) {
        // test aid: dL/d(BN1 output) is not a tensor of the step any more; the tap gets it from the stand-alone data-gradient kernel
        ca.out = nxt; ca.partials = partials;
        if (g8) ca.gin = (unsigned char*)c->grad_tap + (size_t)N * 768 * 2;          // (its bf16 expansion in tap slot 1)
        if (int e = launch_conv2_dgrad<T>(ctx.conv(), ca, &grid_d)) return e;
        ca.gin = cur;
        if (int e = tap_gradient(c, 0, nxt, N, 768, sizeof(T), st)) return e;         // dL/d(BN1 output), [w][c]
    }
    // ---- conv2's data gradient, BatchNorm1 + ReLU backward and conv1's gradients in one pass over cur ------------------
    {
        ca.out = nullptr; ca.partials = partials;
        if (small) {
            // (BatchNorm1's backward is finalised in the kernel's prologue, from the finish launch's rows)
            ca.stats1 = ctx.stats(0); ca.rows1 = ctx.rows2(); ca.rows1_nr = CONV2_FINISH_ROWS;
            ca.dgamma1 = g->bn_g[0]; ca.dbeta1 = g->bn_b[0];
        }
        if (int e = launch_conv2_dgrad_conv1<T>(ctx.conv(), ca, small, g8 != nullptr, &grid_d)) return e;
    }
    if (int e = conv1_bwd_finalize(ctx.conv(), grid_d, g)) return e;
    if (aux) { if (int e = aux->join()) return e; }      // everything the second stream was given is part of this call
    return 0;
}

template <typename T>
static int encoder_backward_small_t(const cp_config* c, const cp_params* p, const float* x, unsigned char* base, const WS& w,
                                    cp_params* g, hipStream_t st, hipEvent_t fc_grads_ready) {
    const Pass ctx(c, base, w, st);
    const int64_t N = c->n_windows;
    const bool drop = ctx.drop();
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
    size_t slab_off = 0;
    SmReduceBatch rb{};
    rb.splits = splits; rb.slab_stride = kSlabStride;
    auto grad_dst = [&](float* real, int numel) -> float* {          // where a role-1 block writes split 0 of this tensor
        if (splits == 1) return real;
        float* sl = ctx.slabs + slab_off;
        rb.job[rb.njobs++] = SmReduceJob{sl, real, numel};
        slab_off += (size_t)numel;
        return sl;
    };
    int cur = 0;
    {
        SmBwdArgs a{};
        a.Gin = base + w.dz; a.Wt = base + w.wlast_t; a.Rp = ctx.act<T>(8); a.stats_p = ctx.stats(8); a.Gout = gb[cur]; a.out_acc = gacc_of(8);
        a.dW = grad_dst(g->last_w, CP_D_E * 512); a.db = nullptr; a.slab_stride = kSlabStride; a.rows_per_split = rps; a.splits = splits;
        a.p_valid = CP_D_E; a.N = N; a.K = 512; a.smod = 512; a.wmode = 0; a.n_dgrad = tiles_m * (512 / bn_tile);
        if (drop) set_dropout(a, ctx, 8);
        ProfScope ps(CP_K_PROJ_BWD, st);
        if (ks) hipLaunchKernelGGL((sm_fc_bwd_kernel<T, true, true>), dim3(a.n_dgrad + 8 * splits), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sm_fc_bwd_kernel<T, true>), dim3(a.n_dgrad + 8 * splits), dim3(256), 0, st, a);
        CKL("sm_fc_bwd_kernel<proj>");
    }
    // gradient tap: every launch's stored data gradient, copied directly behind the launch that wrote it.  Gout is the masked
    // dL/d(BN_L output) -- the NEXT launch applies layer L's BatchNorm + ReLU backward while staging -- so slot L = 2..8 holds that,
    // and fc1's [N][768] goes to slot 9 before conv_backward_tail transforms it in place (slots 1 and 0 are filled there).  Slot 10: the
    // projection launch's own input, dz as the head stored it ([N][64], 16 live columns)
    if (int e = tap_gradient(c, 10, base + w.dz, N, 64, sizeof(T), st)) return e;
    if (int e = tap_gradient(c, 8, gb[cur], N, 512, sizeof(T), st)) return e;
    for (int L = 8; L >= 2; --L) {
        const int i = L - 2, Lp = L - 1, K = fcK(i);
        SmBwdArgs a{};
        a.Gin = gb[cur]; a.R = ctx.act<T>(L); a.gsum = gacc_of(L); a.stats = ctx.stats(L);
        a.dgamma = g->bn_g[L]; a.dbeta = g->bn_b[L]; a.Wt = base + w.wfc_t[i]; a.Rp = ctx.act<T>(Lp); a.stats_p = ctx.stats(Lp);
        a.Gout = gb[cur ^ 1];
        if (Lp == 1) a.out_partials = ctx.partials;          // fc1: partial rows [tiles_m][2][768] for the conv tail's finalize launch
        else a.out_acc = gacc_of(Lp);
        a.dW = grad_dst(g->fc_w[i], 512 * K); a.db = grad_dst(g->fc_b[i], 512);
        a.slab_stride = kSlabStride; a.rows_per_split = rps; a.splits = splits; a.p_valid = 512;
        a.N = N; a.K = K; a.smod = kLayerC[Lp]; a.wmode = i == 0 ? 1 : 0; a.n_dgrad = tiles_m * (K / bn_tile);
        if (drop && Lp >= 5) set_dropout(a, ctx, Lp);
        ProfScope ps(CP_K_FC_DGRAD, st);
        if (ks) hipLaunchKernelGGL((sm_fc_bwd_kernel<T, false, true>), dim3(a.n_dgrad + 8 * (K / 64) * splits), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sm_fc_bwd_kernel<T, false>), dim3(a.n_dgrad + 8 * (K / 64) * splits), dim3(256), 0, st, a);
        CKL("sm_fc_bwd_kernel");
        cur ^= 1;
        if (int e = tap_gradient(c, Lp == 1 ? 9 : Lp, gb[cur], N, K, sizeof(T), st)) return e;
    }
    if (splits > 1) {
        ProfScope ps(CP_K_REDUCE_SLABS, st);
        hipLaunchKernelGGL(sm_reduce_grads_kernel, dim3(96, rb.njobs), dim3(256), 0, st, rb);
        CKL("sm_reduce_grads_kernel");
    }
    // `partials` now holds fc1's partial sums [tiles_m][2][768]: the conv tail finalises conv2's BatchNorm backward from them
    return conv_backward_tail<T>(c, p, x, base, w, g, st, fc_grads_ready, gb[cur], gb[cur ^ 1], false, tiles_m, nullptr, 0, nullptr, true);
}

template <typename T>
static int encoder_backward_t(const cp_config* c, const cp_params* p, const float* x, unsigned char* base, const WS& w,
                              cp_params* g, hipStream_t st, hipEvent_t fc_grads_ready, bool tposed) {
    using D = DT<T>;
    const Pass ctx(c, base, w, st);
    const int64_t N = c->n_windows;
    const bool drop = ctx.drop();
    float *partials = ctx.partials, *slabs = ctx.slabs, *coef = ctx.coef;
    float* praw = (float*)(base + w.praw);
    const int tiles_n = (int)((N + fc_bm<T>() - 1) / fc_bm<T>());
    int gcol_rows = 0;           // partial rows [768] of fc1's data-gradient launch: column sums of dL/d(conv2 pre-activation)
    int stat_rows = tiles_n;     // partial rows holding the BN-backward sums for the next bn_bwd_finalize
    T* dz = (T*)(base + w.dz);
    T* cur = (T*)(base + w.gbuf[0]);
    T* nxt = (T*)(base + w.gbuf[1]);
    bool bn_done = false;           // (see the comment above the fc loop)
    const bool fuse_ok = sizeof(T) == 2 && !opt(c, CP_OPT_UNFUSED_BN_BWD);
    // Second stream (cp_config.aux_stream, round 4): the weight gradients behind a dropout -- the projection's, fc7's + fc6's (one
    // paired launch), fc5's -- float there beside the critical path's ~40 small launches.  Their gradient operands then
    // live in buffers of their own (w.gkeep) instead of the ping-pong, so that no data-gradient launch has to wait for them.
    // (not for the CP_OPT_FP8_BRIDGE test route, which runs this function on a CP_FP8 workspace: its gkeep buffers hold bytes)
    const Aux aux = make_aux(c, st, fuse_ok && drop && !dyn_tiles(c) && !opt(c, CP_OPT_UNPAIRED_WGRAD) && c->dtype != CP_FP8);
    if (aux.on) { cur = (T*)(base + w.gkeep[0]); nxt = (T*)(base + w.gkeep[1]); }
    if (!(aux.on && tposed)) {              // (else made beside the forward pass and waited for by cp_encoder_backward_ev)
        if (int e = launch_weight_transposes<T>(p, base, w, st)) return e;
    }
    if (int e = aux.fork()) return e;           // dz (cp_head) is final
    // ---- projection ------------------------------------------------------------------
    {
        ProfScope ps(CP_K_PROJ_BWD, st);
        const ProjLaunch pl = ctx.proj();
        const float *s = nullptr, *t = nullptr;
        float* dzsum = (float*)(base + w.dzsum);
        if (!drop) {
            s = ctx.scale(8); t = ctx.shift(8);
            if (int e = proj_dz_sums<T>(pl, dz, dzsum)) return e;
        }
        ProjDrop dp{};
        if (drop) set_dropout(dp, ctx, 8);
        const hipStream_t sw = aux.s();                 // (with dropout nothing waits for this weight gradient: second stream)
        int S;
        const bool proj_alg = fuse_ok && drop && sizeof(T) == 2;
        // (proj_dgrad_kernel finalises fc7's BatchNorm backward in its prologue: the finish launch's rows then go to rows2, bwd_in_prologue)
        const bool proj_pro = proj_alg && bwd_in_prologue(ctx, PROJ_FINISH_ROWS, 16);
        if (proj_alg) {
            // behind fc7's dropout, 16-bit storage (round 4): the weight gradient's launch reads r8 ONCE and leaves both dW and fc7's
            // BatchNorm-backward sums (gemm_tn.cuh, proj_wgrad_sums_kernel); on the critical path -- the data gradient below needs the sums
            if constexpr (sizeof(T) == 2) {
                ProjLaunch pw = pl;
                if (proj_pro) pw.partials = ctx.rows2();
                if (int e = launch_proj_wgrad_onepass(pw, (const bf16_t*)dz, ctx.act<T>(8), nullptr, slabs, dp, ctx.scale(8), ctx.shift(8), p->last_w, g->last_w, &S)) return e;
            }
        } else {
            if (int e = launch_proj_wgrad_tn<T>(pl, sw, dz, ctx.act<T>(8), nullptr, aux.on ? (float*)(base + w.slabs_b) : slabs, ctx.scale(8), ctx.shift(8), dp,
                                                s, t, dzsum, g->last_w, drop ? (float*)nullptr : praw, &S)) return e;
        }
        if (!drop) {
            if (int e = proj_sums_from_wgrad(pl, p->last_w, praw, dzsum)) return e;
            stat_rows = 1;
        }
        GemmNTArgs a{};
        a.A = dz; a.lda = 64; a.M = N; a.K = 64;
        a.W = base + w.wlast_t; a.F = 512;
        a.C = cur; a.ldc = 512; a.R = drop ? ctx.act<T>(8) : nullptr; a.ldr = 512; a.partials = partials;
        if (drop) set_dropout(a, ctx, 8);
        int drows = 0;
        if (fuse_ok && !drop) {
            // no dropout behind fc7: its BN-backward sums are known (from the projection's weight gradient), so this
            // launch applies fc7's BN + ReLU backward itself, as the fc launches below do for their layer below
            if (int e = bwd_finalize(ctx, g, partials, stat_rows, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, fused)")) return e;
            a.R = ctx.act<T>(8); a.coef = coef; a.coef_mod = 512;
            CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, &drows, dyn_tiles(c))));
            if (int e = bias_grad_from_rows(ctx, drows, 512, g->fc_b[6], "colsum_finalize_kernel(fc7, fused)")) return e;
            bn_done = true;
        } else if (proj_alg) {
            // behind fc7's dropout: the rank-16 product is formed with fc7's BN + ReLU backward applied (gemm_ws.cuh, proj_dgrad_kernel)
            // instead of being written out for a separate bn_relu_bwd pass; the BatchNorm-backward sums it needs came with the weight
            // gradient above (round 3's first pass of the same product was removed; see git history)
            if (proj_pro) set_bn_prologue(a, ctx, g, ctx.rows2(), PROJ_FINISH_ROWS, (double)N, 8);
            else if (int e = bwd_finalize(ctx, g, partials, PROJ_FINISH_ROWS, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, projection)")) return e;
            a.coef = coef; a.coef_mod = 512;
            CK(launch_proj_dgrad(a, st, &drows));
            if (int e = bias_grad_from_rows(ctx, drows, 512, g->fc_b[6], "colsum_finalize_kernel(fc7, projection)")) return e;
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
    struct { const T* X; const T* Y; int i; } pend{};     // a weight gradient waiting for the next layer's (place_wgrad, defer)
    bool pending = false;
    for (int L = 8; L >= 2; --L) {
        const int i = L - 2, Lp = L - 1, K = fcK(i);
        if (!bn_done) {
            ProfScope ps(CP_K_BN_BWD, st);
            int nr = stat_rows;
            const float* pp = ctx.pre(nr, 2 * 512);
            if (int e = bwd_finalize(ctx, g, pp, nr, (double)N, L, 512, 1, "bn_bwd_finalize_kernel")) return e;
            const int gb = launch_bn_relu_bwd<T>(cur, ctx.act<T>(L), coef, partials, N, 512, CAP_BRB16, st);
            // (the bias gradient is consumed within this pass -- reduce_slabs' BatchNorm un-fold and
            //  bn_bwd_sums_from_wgrad_kernel read it -- so these small launches cannot be batched at the end of the loop)
            if (int e = bias_grad_from_rows(ctx, gb, 512, g->fc_b[i], "bn_relu_bwd_kernel")) return e;
        }
        if (int e = tap_gradient(c, L, cur, N, 512, sizeof(T), st)) return e;        // dL/d(pre-activation of layer L)
        const bool in_drop = drop && Lp >= 5;
        const T* Y = in_drop ? (const T*)(base + w.u[Lp - 5]) : ctx.act<T>(Lp);
        const float* s = in_drop ? nullptr : ctx.scale(Lp);
        const float* t = in_drop ? nullptr : ctx.shift(Lp);
        // the fused data gradient below runs gemm_wsd16_kernel<0> (launch_fc_gemm: 16 bits, static schedule), which finalises layer Lp's
        // BatchNorm backward in its prologue: the sums' rows then go to rows2 (bwd_in_prologue)
        const bool dgrad_pro = fuse_ok && !in_drop && !dyn_tiles(c) && bwd_in_prologue(ctx, kSumSlices, 16);
        int S;
        WgradPlace pl;           // (paired launches: 16-bit storage only, and not under CP_OPT_UNPAIRED_WGRAD)
        if (int e = place_wgrad(ctx, aux, in_drop, i, sizeof(T) == 2 && !opt(c, CP_OPT_UNPAIRED_WGRAD), &pl)) return e;
        if (pl.defer) {
            pend.X = cur; pend.Y = Y; pend.i = i;
            pending = true;
        } else if constexpr (sizeof(T) == 2) {
            // 256x256 tiles: 4 (K=512) or 6 (K=768) tiles x ~256/tiles splits = one block per CU
            GemmTN256Args ta{};
            ta.X = (const bf16_t*)cur; ta.ldx = 512; ta.Y = (const bf16_t*)Y; ta.ldy = K; ta.slabs = pl.slabs; ta.M = N; ta.P = 512; ta.Q = K;
            if (pending) { ta.X2 = (const bf16_t*)pend.X; ta.Y2 = (const bf16_t*)pend.Y; ta.slabs2 = pl.slabs + (size_t)32 * 512 * 512; }
            split_rows(N, pending ? 32 : (K == 512 ? 64 : 40), &S, &ta.rows_per_split);
            ta.splits = S;
            ProfScope ps(CP_K_FC_WGRAD, pl.sw);
            CK(launch_gemm_tn256(ta, pl.sw));
        } else {
            GemmTNArgs ta{};
            ta.X = cur; ta.ldx = 512; ta.Y = Y; ta.ldy = K; ta.slabs = slabs; ta.M = N; ta.P = 512; ta.Q = K;
            split_rows(N, 32, &S, &ta.rows_per_split);
            ProfScope ps(CP_K_FC_WGRAD, st);
            CK((launch_gemm_tn<T, 128, 128, YLOAD_PLAIN>(ta, S, st)));
        }
        if (!pl.defer) {
            ProfScope ps(CP_K_REDUCE_SLABS, pl.sw);
            if (pending && !opt(c, CP_OPT_FINALIZE_LAUNCHES)) {
                // the deferred layer (always behind a dropout: no BN fold to undo, no raw product wanted) and this one in one launch
                ReduceSlabsPair rp{};
                rp.job[0] = ReduceSlabsJob{pl.slabs + (size_t)32 * 512 * 512, nullptr, nullptr, g->fc_b[pend.i], g->fc_w[pend.i], nullptr, S, 512, 512, 512, 0};
                rp.job[1] = ReduceSlabsJob{pl.slabs, s, t, g->fc_b[i], g->fc_w[i], in_drop ? (float*)nullptr : praw, S, 512, K, 512, i == 0 ? 1 : 0};
                hipLaunchKernelGGL(reduce_slabs_pair_kernel, dim3(512, 2), dim3(256), 0, pl.sw, rp);
                CKL("reduce_slabs_pair(fc)");
                pending = false;
            } else {
                if (pending) {
                    // the deferred layer (always behind a dropout: no BN fold to undo, no raw product wanted)
                    hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(512), dim3(256), 0, pl.sw, pl.slabs + (size_t)32 * 512 * 512, S, 512, 512, 512,
                                       (const float*)nullptr, (const float*)nullptr, g->fc_b[pend.i], g->fc_w[pend.i], 0, (float*)nullptr);
                    CKL("reduce_slabs(fc, deferred)");
                    pending = false;
                }
                hipLaunchKernelGGL(reduce_slabs_kernel<float>, dim3(512), dim3(256), 0, pl.sw, pl.slabs, S, 512, K, 512, s, t, g->fc_b[i], g->fc_w[i],
                                   i == 0 ? 1 : 0, in_drop ? (float*)nullptr : praw);
                CKL("reduce_slabs(fc)");
            }
            if (!in_drop) {
                // no dropout between this layer and the previous BN: its backward sums follow from P = g_y^T r
                // (just reduced), W and db -- the data-gradient launch below then reads no saved activation
                hipLaunchKernelGGL(bn_bwd_sums_from_wgrad_kernel, dim3(K / 64, kSumSlices), dim3(256), 0, st, praw, p->fc_w[i],
                                   g->fc_b[i], dgrad_pro ? ctx.rows2() : partials, 512, K, i == 0 ? 1 : 0);
                CKL("bn_bwd_sums_from_wgrad_kernel");
            }
        }
        stat_rows = in_drop ? tiles_n : kSumSlices;
        GemmNTArgs a{};
        a.A = cur; a.lda = 512; a.M = N; a.K = 512;
        a.W = base + w.wfc_t[i]; a.F = K;
        a.C = nxt; a.ldc = K; a.R = in_drop ? ctx.act<T>(Lp) : nullptr; a.ldr = K; a.partials = partials;
        if (in_drop) set_dropout(a, ctx, Lp);
        bn_done = false;
        if (fuse_ok && !in_drop) {
            // layer Lp's BN-backward sums exist already (from the weight gradient above): finalise its coefficients
            // now and let this launch's epilogue apply BN backward + the ReLU mask to its own output tile
            const int Cp = kLayerC[Lp], nfold = K / Cp;                   // fc below: 512 x 1; conv2 below: 64 x 12
            {
                // (the profiler keeps its record of this step of the plan; with the prologue it brackets no launch)
                ProfScope ps(CP_K_BN_BWD, st);
                int nr = stat_rows;
                const float* pp = ctx.pre(nr, 2 * K);
                if (dgrad_pro) set_bn_prologue(a, ctx, g, ctx.rows2(), nr, (double)N * nfold, Lp);
                else if (int e = bwd_finalize(ctx, g, pp, nr, (double)N * nfold, Lp, Cp, nfold, "bn_bwd_finalize_kernel(fused)")) return e;
            }
            a.R = ctx.act<T>(Lp); a.coef = coef; a.coef_mod = Cp;
            int drows = 0;
            {
                ProfScope ps(CP_K_FC_DGRAD_BN, st);                        // data gradient + BN/ReLU backward of the layer below
                CK((launch_fc_gemm<T, EPI_DGRAD>(a, st, &drows, dyn_tiles(c))));
            }
            if (Lp == 1) gcol_rows = drows;                               // (the conv tail reads these bias-gradient rows once more)
            {
                ProfScope ps(CP_K_BN_BWD, st);                            // rows of K = nfold rows of Cp
                if (int e = bias_grad_from_rows(ctx, drows * nfold, Cp, Lp >= 2 ? g->fc_b[i - 1] : g->conv2_b, "colsum_finalize_kernel(fused)")) return e;
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
        rotate_grads(cur, nxt, aux.on, L, (T*)(base + w.gkeep[2]), (T*)(base + w.gbuf[0]), (T*)(base + w.gbuf[1]));
    }
    return conv_backward_tail<T>(c, p, x, base, w, g, st, fc_grads_ready, cur, nxt, bn_done, stat_rows, &aux, gcol_rows, nullptr, false);
}

// ---------------------------------------------------------------------------------------
// encoder backward, CP_FP8: the fc stack in 8 bits (csrc/fp8.cuh) -- e5m2 gradients between the layers, the saved e4m3
// activations, W^T as e4m3 -- then the conv stack on the bf16 kernels (fc1's data-gradient launch writes e5m2 bytes they expand).
// Same order of work as encoder_backward_t<bf16_t>, from the same pieces; CP_OPT_FP8_BRIDGE (cp_config.options) keeps the first
// build's route (fp8_bridge_expand, then the bf16 backward) for A/B runs and for the test that compares the two.
// ---------------------------------------------------------------------------------------
static int encoder_backward_fp8(const cp_config* c, const cp_params* p, const float* x, unsigned char* base, const WS& w,
                                cp_params* g, hipStream_t st, hipEvent_t fc_grads_ready, bool tposed) {
    using T = bf16_t;
    const Pass ctx(c, base, w, st);
    const int64_t N = c->n_windows;
    const bool drop = ctx.drop();
    float *partials = ctx.partials, *slabs = ctx.slabs, *coef = ctx.coef;
    float* praw = (float*)(base + w.praw);
    Fp8State* fs = (Fp8State*)(base + w.f8state);
    auto tap8 = [&](int slot, const uint8_t* src, int t) -> int {          // test aid: the e5m2 gradient expanded into the bf16 tap
        if (!c->grad_tap) return 0;
        const size_t slot_bytes = (size_t)N * 768 * 2;
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
    // (these sums are in true units on this path, so synchronised BatchNorm's rows cross the ranks as they are)
    const Aux aux = make_aux(c, st, drop);
    if (aux.on) { cur = base + w.gkeep[0]; nxt = base + w.gkeep[1]; }
    if (!(aux.on && tposed)) {
        if (int e = launch_weight_transposes_fp8(p, base, w, st)) return e;
    }
    if (int e = aux.fork()) return e;
    // ---- projection ------------------------------------------------------------------
    {
        ProfScope ps(CP_K_PROJ_BWD, st);
        const ProjLaunch pl = ctx.proj();
        float* dzsum = (float*)(base + w.dzsum);
        if (!drop) {
            if (int e = proj_dz_sums<T>(pl, dz, dzsum)) return e;
        }
        int S;
        if (drop) {
            // (encoder_backward_t: one pass over r8 for the weight gradient AND fc7's BatchNorm-backward sums, on the critical path)
            ProjDrop dp{};
            set_dropout(dp, ctx, 8);
            if (int e = launch_proj_wgrad_onepass(pl, (const bf16_t*)dz, ctx.act8(8), (const int*)&fs->e[F8_T_ACT + 8], slabs, dp, ctx.scale(8), ctx.shift(8),
                                                  p->last_w, g->last_w, &S)) return e;
        } else {
            if (int e = launch_proj_wgrad_tn<T>(pl, aux.s(), dz, ctx.act8(8), &fs->e[F8_T_ACT + 8], aux.on ? (float*)(base + w.slabs_b) : slabs, nullptr, nullptr,
                                                ProjDrop{}, ctx.scale(8), ctx.shift(8), dzsum, g->last_w, praw, &S)) return e;
        }
        Proj8Args a{};
        a.A = dz; a.lda = 64; a.W = (const bf16_t*)(base + w.wlast_t); a.K = 64; a.R = ctx.act8(8); a.C = cur;
        a.partials = partials; a.st = fs; a.t_r = F8_T_ACT + 8; a.t_out = F8_T_GRAD + 8; a.M = N;
        int drows = 0;
        if (drop) {
            set_dropout(a, ctx, 8);
            if (int e = bwd_finalize(ctx, g, partials, PROJ_FINISH_ROWS, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, projection)")) return e;
        } else {
            if (int e = proj_sums_from_wgrad(pl, p->last_w, praw, dzsum)) return e;
            if (int e = bwd_finalize(ctx, g, partials, 1, (double)N, 8, 512, 1, "bn_bwd_finalize_kernel(fc7, fused)")) return e;
        }
        a.coef = coef;
        CK(launch_proj_dgrad8(a, st, &drows));
        if (int e = bias_grad_from_rows(ctx, drows, 512, g->fc_b[6], "colsum_finalize_kernel(fc7)")) return e;
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
            const float* pp = ctx.pre(nr, 2 * 512);
            if (int e = bwd_finalize(ctx, g, pp, nr, (double)N, L, 512, 1, "bn_bwd_finalize_kernel")) return e;
            const int gb = launch_bn_relu_bwd8(cur, ctx.act8(L), coef, partials, N, fs, F8_T_GB + L, F8_T_ACT + L, F8_T_GRAD + L, st);
            if (int e = bias_grad_from_rows(ctx, gb, 512, g->fc_b[i], "bn_relu_bwd8_kernel")) return e;
        }
        if (int e = tap8(L, cur, F8_T_GRAD + L)) return e;
        const bool in_drop = drop && Lp >= 5;
        const uint8_t* Y = in_drop ? base + w.u8[Lp - 5] : ctx.act8(Lp);
        const int ty = in_drop ? F8_T_U + (Lp - 5) : F8_T_ACT + Lp, tx = F8_T_GRAD + L;
        const float* s = in_drop ? nullptr : ctx.scale(Lp);
        const float* t = in_drop ? nullptr : ctx.shift(Lp);
        int S;
        WgradPlace pl;
        if (int e = place_wgrad(ctx, aux, in_drop, i, true, &pl)) return e;
        if (pl.defer) {
            pend.X = cur; pend.Y = Y; pend.i = i; pend.tx = tx; pend.ty = ty;
            pending = true;
        } else {
            GemmTN8Args ta{};
            ta.X = cur; ta.ldx = 512; ta.Y = Y; ta.ldy = K; ta.slabs = pl.slabs; ta.M = N; ta.P = 512; ta.Q = K;
            // (32 splits for the single-layer launches too -- half the slab bytes, half the blocks -- measured: weight gradients 5 x 67 -> 82 us,
            //  slab reductions 9 x 11.0 -> 9.1: 70 us lost for 17 gained)
            split_rows_tn8(N, pending, K, &S, &ta.rows_per_split);
            if (pending) { ta.X2 = pend.X; ta.Y2 = pend.Y; ta.slabs2 = pl.slabs + (size_t)32 * 512 * 512; }
            ta.splits = S;
            ProfScope ps(CP_K_FC_WGRAD, pl.sw);
            CK(launch_gemm_tn8(ta, pl.sw));
        }
        if (!pl.defer) {
            ProfScope ps(CP_K_REDUCE_SLABS, pl.sw);
            if (pending) {
                launch_reduce_slabs8(pl.slabs + (size_t)32 * 512 * 512, S, 512, nullptr, nullptr, g->fc_b[pend.i], g->fc_w[pend.i], 0, nullptr,
                                     (const int*)&fs->e[pend.tx], (const int*)&fs->e[pend.ty], pl.sw);
                CKL("reduce_slabs(fc, deferred)");
                pending = false;
            }
            launch_reduce_slabs8(pl.slabs, S, K, s, t, g->fc_b[i], g->fc_w[i], i == 0 ? 1 : 0, in_drop ? (float*)nullptr : praw,
                                 (const int*)&fs->e[tx], (const int*)&fs->e[ty], pl.sw);
            CKL("reduce_slabs(fc)");
            if (!in_drop) {
                hipLaunchKernelGGL(bn_bwd_sums_from_wgrad_kernel, dim3(K / 64, kSumSlices), dim3(256), 0, st, praw, p->fc_w[i], g->fc_b[i],
                                   partials, 512, K, i == 0 ? 1 : 0);
                CKL("bn_bwd_sums_from_wgrad_kernel");
            }
        }
        Wsd8Args a{};
        a.A = cur; a.W = base + w.wfc8t[i]; a.wsc = base + w.wsc8t[i]; a.R = ctx.act8(Lp); a.partials = partials;
        a.st = fs; a.t_r = F8_T_ACT + Lp; a.M = N; a.F = K;
        bn_done = false;
        if (!in_drop) {
            const int Cp = kLayerC[Lp], nfold = K / Cp;
            {
                ProfScope ps(CP_K_BN_BWD, st);
                int nr = kSumSlices;
                const float* pp = ctx.pre(nr, 2 * K);
                if (int e = bwd_finalize(ctx, g, pp, nr, (double)N * nfold, Lp, Cp, nfold, "bn_bwd_finalize_kernel(fused)")) return e;
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
                if (int e = bias_grad_from_rows(ctx, drows * nfold, Cp, Lp >= 2 ? g->fc_b[i - 1] : g->conv2_b, "colsum_finalize_kernel(fused)")) return e;
            }
            bn_done = true;
        } else {
            // (the dropout OUTPUT of layer Lp stands in for its saved activation: its zeros are the mask -- fp8.cuh, MODE 1)
            a.C = nxt; a.t_out = F8_T_GB + Lp;
            a.R = base + w.u8[Lp - 5]; a.t_r = F8_T_U + (Lp - 5); a.bn_stats = ctx.stats(Lp); a.dp_inv_keep = dp_inv_keep(c->dp_emg);
            ProfScope ps(CP_K_FC_DGRAD_STATS, st);
            int drows = 0;
            CK((launch_gemm_wsd8<1>(a, st, &drows)));
            stat_rows = drows;
        }
        rotate_grads(cur, nxt, aux.on, L, base + w.gkeep[2], base + w.g8[0], base + w.g8[1]);
    }
    return conv_backward_tail<T>(c, p, x, base, w, g, st, fc_grads_ready, gconv, (T*)(base + w.gbuf[1]), true, 0, &aux, gcol_rows, fs, false);
}

// CP_OPT_FP8_BRIDGE: the e4m3 tensors of a CP_FP8 forward pass expanded to bf16 -- exactly -- where the bf16 backward kernels read them
static int fp8_bridge_expand(const Pass& ctx) {
    const WS& w = ctx.w;
    const Fp8State* fs = (const Fp8State*)(ctx.base + w.f8state);
    const int64_t N = ctx.N();
    for (int l = 1; l < CP_N_BN; ++l) {
        const int64_t n16 = N * (l < 2 ? 768 : 512) / 16;
        hipLaunchKernelGGL(dequant8_bf16_kernel, dim3(grid_rows(n16, 256, 4096)), dim3(256), 0, ctx.st, ctx.act8(l), ctx.act<bf16_t>(l), n16, fs, F8_T_ACT + l);
    }
    if (ctx.drop())
        for (int i = 0; i < 3; ++i)
            hipLaunchKernelGGL(dequant8_bf16_kernel, dim3(grid_rows(N * 32, 256, 4096)), dim3(256), 0, ctx.st, ctx.base + w.u8[i], (bf16_t*)(ctx.base + w.u[i]), N * 32, fs, F8_T_U + i);
    CKL("dequant8_bf16_kernel");
    return 0;
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
    if (int e = check_tap(cfg, r->path == PATH_SMALL)) return e;
    unsigned char* base = (unsigned char*)ws;
    const hipStream_t st = (hipStream_t)stream;
    const hipEvent_t ready = (hipEvent_t)fc_grads_ready;
    const int repeats = r->backwards++;
    const bool tposed = r->transposed != 0;
    // the transposed weights made beside the forward pass (cp_encoder_forward) precede every launch of this call, whether or not this
    // call uses the second stream itself
    if (tposed) CK(hipStreamWaitEvent(st, (hipEvent_t)r->join_event, 0));
    if (use_small(cfg)) {
        if (repeats > 0) {
            // a second backward over the same forward: the small-batch form's BatchNorm-backward totals (fixed-point atomics, zeroed by the
            // forward's preparation launch) already hold the first pass's sums
            CK(hipMemsetAsync(base + w.sm_acc + (size_t)9 * 2 * 768 * 8, 0, (size_t)9 * 2 * 768 * 8, st));
        }
        return by_dtype(cfg->dtype, [&](auto tag) { return encoder_backward_small_t<typename decltype(tag)::type>(cfg, p, x, base, w, grads, st, ready); });
    }
    if (cfg->dtype == CP_FP8 && !opt(cfg, CP_OPT_FP8_BRIDGE)) return encoder_backward_fp8(cfg, p, x, base, w, grads, st, ready, tposed);
    if (cfg->dtype == CP_FP8) {
        if (int e = fp8_bridge_expand(Pass(cfg, base, w, st))) return e;
        return encoder_backward_t<bf16_t>(cfg, p, x, base, w, grads, st, ready, false);
    }
    return by_dtype(cfg->dtype, [&](auto tag) { return encoder_backward_t<typename decltype(tag)::type>(cfg, p, x, base, w, grads, st, ready, tposed); });
}

extern "C" int cp_encoder_backward(const cp_config* cfg, const cp_params* p, const float* x, void* ws, size_t ws_bytes,
                                   cp_params* grads, void* stream) {
    return cp_encoder_backward_ev(cfg, p, x, ws, ws_bytes, grads, stream, nullptr);
}

// ---------------------------------------------------------------------------------------
// debug access to what a pass left in the workspace
// ---------------------------------------------------------------------------------------
extern "C" int cp_debug_activation(const cp_config* cfg, const cp_params* p, const float* x, void* ws, size_t ws_bytes,
                                   int32_t layer, float* out, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (layer < 0 || layer >= CP_N_BN + 4 || !out) return fail(CP_ERR_ARG, "cp_debug_activation args");
    if (layer >= CP_N_BN && !(cfg->dp_emg > 0.f)) return fail(CP_ERR_ARG, "dropout buffers exist only when dp_emg > 0");
    const int64_t N = cfg->n_windows, n = N * (layer < 2 ? 768 : 512);
    unsigned char* base = (unsigned char*)ws;
    const hipStream_t st = (hipStream_t)stream;
    if (layer == 0) {   // conv1's output is never stored: recompute it exactly as its consumers do
        if (!p || !x) return fail(CP_ERR_ARG, "layer 0 needs params and x");
        by_dtype(cfg->dtype, [&](auto tag) {
            hipLaunchKernelGGL((conv1_materialize_kernel<typename decltype(tag)::type>), dim3(1024), dim3(256), 0, st, x, p->conv1_w, p->conv1_b, out, N * 12);
            return 0;
        });
        CKL("conv1_materialize_kernel");
        return 0;
    }
    if (cfg->dtype == CP_FP8) {
        // the stored e4m3 tensor in true units (dropout(BN(fc7)), layer CP_N_BN + 3, is never stored on this path)
        if (layer == CP_N_BN + 3) {
            // dropout(BN(fc7)) is formed while staging and never stored: computed here in f32 from the stored e4m3 activation, same key
            hipLaunchKernelGGL(debug_bn_dropout8_f32_kernel, dim3(1024), dim3(256), 0, st, base + w.act8[8],
                               (const float*)(base + w.stats[8]), out, N, 512, dp_thresh(cfg->dp_emg), dp_key(cfg, 8),
                               dp_inv_keep(cfg->dp_emg), dp_salt(cfg), (const Fp8State*)(base + w.f8state), F8_T_ACT + 8);
            CKL("debug_bn_dropout8_f32_kernel");
            return 0;
        }
        const int t = layer < CP_N_BN ? F8_T_ACT + layer : F8_T_U + (layer - CP_N_BN);
        const uint8_t* src = base + (layer < CP_N_BN ? w.act8[layer] : w.u8[layer - CP_N_BN]);
        hipLaunchKernelGGL(dequant8_f32_kernel, dim3(1024), dim3(256), 0, st, src, out, n, (const Fp8State*)(base + w.f8state), t);
        CKL("dequant8_f32_kernel");
        return 0;
    }
    const size_t off = layer < CP_N_BN ? w.act[layer] : w.u[layer - CP_N_BN];
    // dropout(BN(.)) of fc4..fc6 is STORED by the large-batch forward: read what it stored.  fc7's (formed while staging, never
    // written) and all four after a small-batch forward (csrc/small.cuh applies BatchNorm + dropout while staging) are recomputed from
    // the stored activation with the forward pass's key, into the otherwise unused buffer.
    const bool stored_u = layer >= CP_N_BN && layer < CP_N_BN + 3 &&
                          (cfg->record && cfg->record->n_windows ? cfg->record->path : forward_path(cfg)) == PATH_LARGE;
    return by_dtype(cfg->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (layer >= CP_N_BN && !stored_u) {
            const int Lp = 5 + (layer - CP_N_BN);
            hipLaunchKernelGGL((bn_dropout_apply_kernel<T>), dim3(grid_rows(N, 256 / (512 / DT<T>::EPC), 4096)), dim3(256), 0, st,
                               (const T*)(base + w.act[Lp]), (const float*)(base + w.stats[Lp]), (T*)(base + off), N, 512, dp_thresh(cfg->dp_emg),
                               dp_key(cfg, Lp), dp_inv_keep(cfg->dp_emg), dp_salt(cfg));
            CKL("bn_dropout_apply_kernel(debug)");
        }
        hipLaunchKernelGGL((to_f32_kernel<T>), dim3(1024), dim3(256), 0, st, (const T*)(base + off), out, n);
        CKL("to_f32_kernel");
        return 0;
    });
}

extern "C" int cp_debug_bn_stats(const cp_config* cfg, void* ws, size_t ws_bytes, int32_t layer, float* out, void* stream) {
    WS w;
    if (int e = check_cfg(cfg, ws, ws_bytes, &w)) return e;
    if (layer < 0 || layer >= CP_N_BN || !out) return fail(CP_ERR_ARG, "cp_debug_bn_stats args");
    CK(hipMemcpyAsync(out, (unsigned char*)ws + w.stats[layer], (size_t)4 * kLayerC[layer] * 4, hipMemcpyDeviceToDevice,
                      (hipStream_t)stream));
    return 0;
}
