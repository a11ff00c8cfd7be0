// Host layer of the online decoders (include/cpnative.h, cp_online_*): workspace layout, argument checks, launch chains and
// the extern "C" entries of the folded, adaptive, multi-stream and adaptive multi-stream decoders, class enrolment, head
// fine-tuning, the command gate, the sequence decoder and its sweep, the grasp drive, the gate sweep, the subset sweep, the electrode-map sweep, cue realignment, prototype
// tracking, held-out enrolment scoring, posture prototypes, the user metric, the closed-form head fit and the per-stream projections of the multi-stream forms.  Host code only; api.hip includes it behind its own helpers (fail, CK, CKL) and encoder_api.cuh's (align256, fcK),
// so the library stays one translation unit.  The four decoders share one workspace description (OlWS, ol_carve), one
// parameter check, one set of front-end arguments, one folded chain and one unfolded weight copy; what an entry adds is its
// name in the refusals and the kernels it launches.
#pragma once
#include <type_traits>

static_assert(OL_MAXM == CP_ONLINE_MAX_WINDOWS && OL_MAXVOTE == CP_ONLINE_MAX_VOTE && OL_MAXK == CP_ONLINE_MAX_CLASSES, "online limits");
static_assert(OLM_MAXS == CP_ONLINE_MULTI_MAX_STREAMS && OL_MAXK == 64, "multi-stream limits");
static_assert(OLAM_STATS == CP_N_BN * 2 * OLA_F, "one stream's statistics: mu and v of every BatchNorm");

// "<who>: <what>" as cp_last_error reports a refusal of entry (or family) `who`
static int ol_fail(int code, const char* who, const char* what) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return fail(code, msg);
}

// f(T()) with T the compute type of `dtype`; the *_t functions below take that value as their first argument
template <typename F>
static int ol_dispatch(int dtype, F f) {
    return dtype == CP_BF16 ? f(bf16_t()) : f(float());
}

// ---------------------------------------------------------------------------------------
// the workspace of all four decoders.  Members a form does not have are not taken (and stay 0).  Three things hold for every
// form: `state` is at offset 0 (cp_online_set_classes / cp_online_reset take an adaptive workspace, the multi entries a
// multi-adaptive one); in the multi forms the OlmMeta array follows the states directly; every block starts 256-aligned, so
// the total does not depend on the order of the blocks.
// ---------------------------------------------------------------------------------------
struct OlWS {
    size_t state, meta, head, stats;     // per stream: OlState; multi: OlmMeta; adaptive: OlaHead and the float64 statistics
    size_t c1w, c1b, c2w, c2b, fcw[CP_N_FC], fcb[CP_N_FC], pw, pb, gb;     // the weights once; gb (adaptive): gamma and beta
    size_t X, C1, R2, H0, H1;            // `rows` rows; C1, R2 (adaptive): conv2's operand, rows (window, position), and its f32 output
    size_t total;
};
// rows: windows of one push (single forms: max_windows; multi forms: max_rows)
static OlWS ol_carve(int64_t rows, int dtype, int n_streams, bool adaptive, bool multi) {
    const size_t es = dtype == CP_BF16 ? 2 : 4, S = (size_t)n_streams;
    const size_t R = (size_t)((rows + 15) / 16 * 16);
    OlWS w{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    w.state = take(S * sizeof(OlState));
    if (multi) w.meta = take(S * sizeof(OlmMeta));
    if (adaptive) {
        w.head = take(S * sizeof(OlaHead));
        w.stats = take(S * OLAM_STATS * 8);
    }
    w.c1w = take(64 * 3 * 4);
    w.c1b = take(64 * 4);
    w.c2w = take(64 * OL_CONV_K * es);
    w.c2b = take((adaptive ? 1 : OL_C) * 64 * 4);          // folded: BN1's shift depends on the position
    for (int i = 0; i < CP_N_FC; ++i) {
        w.fcw[i] = take((size_t)512 * fcK(i) * es);
        w.fcb[i] = take(512 * 4);
    }
    w.pw = take(CP_D_E * 512 * es);
    w.pb = take(CP_D_E * 4);                              // adaptive: zeros (the tail adds a bias the unfolded projection does not have)
    if (adaptive) w.gb = take((size_t)CP_N_BN * 2 * OLA_F * 4);
    w.X = take(R * OL_C * 4);
    if (adaptive) {
        w.C1 = take(R * OL_C * OL_CONV_K * es);
        w.R2 = take(R * OL_C * 64 * 4);
    }
    w.H0 = take(R * 768 * es);
    w.H1 = take(R * 512 * es);
    w.total = o;
    return w;
}

// the view of stream s of an adaptive multi-stream workspace: its state, head and statistics, the shared weights and buffers
static OlWS ol_stream(OlWS w, int s) {
    w.state += (size_t)s * sizeof(OlState);
    w.head += (size_t)s * sizeof(OlaHead);
    w.stats += (size_t)s * OLAM_STATS * 8;
    return w;
}

static int ol_check_config(const cp_online_config* c, void* ws) {
    if (!c || !ws) return fail(CP_ERR_ARG, "cp_online: config and workspace are required");
    if (c->dtype != CP_F32 && c->dtype != CP_BF16) return fail(CP_ERR_ARG, "cp_online: dtype must be CP_F32 or CP_BF16 (no 8-bit path)");
    if (c->max_windows < 1 || c->max_windows > CP_ONLINE_MAX_WINDOWS) return fail(CP_ERR_ARG, "cp_online: max_windows outside 1..256");
    if (c->vote < 1 || c->vote > CP_ONLINE_MAX_VOTE) return fail(CP_ERR_ARG, "cp_online: vote outside 1..256");
    if (c->phase < 0 || c->phase >= CP_ONLINE_STRIDE) return fail(CP_ERR_ARG, "cp_online: phase outside 0..19");
    if (c->n_coef < 2 || c->n_coef > OL_MAXCOEF || c->a[0] == 0.0) return fail(CP_ERR_ARG, "cp_online: IIR coefficients");
    if ((uintptr_t)ws % 256) return fail(CP_ERR_ARG, "cp_online: workspace not 256-byte aligned");
    return 0;
}

// the single-stream forms.  An adaptive workspace too small even for the folded form is refused in the folded form's words.
static int ol_check(const cp_online_config* c, void* ws, size_t ws_bytes, bool adaptive, OlWS* out) {
    if (int e = ol_check_config(c, ws)) return e;
    *out = ol_carve(c->max_windows, c->dtype, 1, false, false);
    if (ws_bytes < out->total) return fail(CP_ERR_WORKSPACE, "cp_online: workspace too small");
    if (!adaptive) return 0;
    *out = ol_carve(c->max_windows, c->dtype, 1, true, false);
    if (ws_bytes < out->total) return fail(CP_ERR_WORKSPACE, "cp_online_adapt: workspace too small");
    return 0;
}

// the multi-stream forms; out: stream 0's view
static int olm_check(const cp_online_config* c, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes, bool adaptive, OlWS* out) {
    const char* who = adaptive ? "cp_online_multi_adapt" : "cp_online_multi";
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return ol_fail(CP_ERR_ARG, who, "n_streams outside 1..256");
    if (max_rows < 1 || max_rows > CP_ONLINE_MULTI_MAX_ROWS) return ol_fail(CP_ERR_ARG, who, "max_rows outside 1..65536");
    if (int e = ol_check_config(c, ws)) return e;
    *out = ol_carve(max_rows, c->dtype, n_streams, adaptive, true);
    if (ws_bytes < out->total) return ol_fail(CP_ERR_WORKSPACE, who, "workspace too small");
    return 0;
}

static int ol_check_index(const char* who, int32_t index, int32_t n_streams) {
    if (index < 0 || index >= n_streams) return ol_fail(CP_ERR_ARG, who, "stream index outside 0..n_streams-1");
    return 0;
}

// an entry of the adaptive multi-stream form that works on one stream; out: that stream's view
static int olam_check_stream(const char* who, const cp_online_config* c, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                             int32_t index, OlWS* out) {
    if (int e = olm_check(c, n_streams, max_rows, ws, ws_bytes, true, out)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    *out = ol_stream(*out, index);
    return 0;
}

// the model a prepare entry takes.  running_required: the folded forms (stock BatchNorm only); else bn may be NULL
static int ol_check_params(const char* who, const cp_params* p, const cp_bn_buffers* bn, bool running_required) {
    const char* stock = "stock BatchNorm with running statistics required (AdaBN has none)";
    bool layers = p && p->conv1_w && p->conv1_b && p->conv2_w && p->conv2_b && p->last_w;
    for (int i = 0; layers && i < CP_N_FC; ++i) layers = p->fc_w[i] && p->fc_b[i];
    if (!layers) return ol_fail(CP_ERR_ARG, who, "parameters");
    if (running_required && !bn) return ol_fail(CP_ERR_ARG, who, stock);
    for (int l = 0; l < CP_N_BN; ++l) {
        if (!p->bn_g[l] || !p->bn_b[l]) return ol_fail(CP_ERR_ARG, who, running_required ? stock : "parameters");
        if (bn && (!bn->running_mean[l] || !bn->running_var[l])) return ol_fail(CP_ERR_ARG, who, running_required ? stock : "running statistics");
    }
    return 0;
}

// what the pushes of the single-stream forms check alike; n == 0 is a valid empty call (the caller returns 0)
static int ol_check_push(const char* who, const cp_online_config* c, int64_t n, const float* raw, const float* mean_std,
                         const int32_t* pred, const int32_t* voted) {
    if (n < 0 || n > (int64_t)CP_ONLINE_STRIDE * c->max_windows) return ol_fail(CP_ERR_ARG, who, "a push takes at most 20 * max_windows samples");
    if (n == 0) return 0;
    if (!raw || !mean_std || !pred || !voted) return ol_fail(CP_ERR_ARG, who, "raw, mean_std, pred and voted are required");
    if ((uintptr_t)raw % 4 || (uintptr_t)mean_std % 4) return ol_fail(CP_ERR_ARG, who, "misaligned input");
    return 0;
}

// the same for the multi-stream forms; total_samples == 0 is a valid empty call
static int olm_check_push(const char* who, int32_t max_rows, const float* raw, const int32_t* counts, int64_t total_samples,
                          int32_t total_windows, const float* mean_std, const int32_t* pred, const int32_t* voted) {
    if (total_windows < 0 || total_windows > max_rows) return ol_fail(CP_ERR_ARG, who, "total_windows outside 0..max_rows");
    if (total_samples < 0) return ol_fail(CP_ERR_ARG, who, "negative total_samples");
    if (total_samples == 0) return 0;
    if (!raw || !counts || !mean_std) return ol_fail(CP_ERR_ARG, who, "raw, counts and mean_std are required");
    if (total_windows > 0 && (!pred || !voted)) return ol_fail(CP_ERR_ARG, who, "pred and voted are required");
    if ((uintptr_t)raw % 4 || (uintptr_t)mean_std % 4 || (uintptr_t)counts % 4) return ol_fail(CP_ERR_ARG, who, "misaligned input");
    return 0;
}

// An electrode map (include/cpnative.h): `rows` rows of 12 sources and 12 fills in memory the device reads, both pointers or
// neither (the identity).  Pinned host memory is checked here: src in -1..11, fill finite.  Device memory the host cannot
// see, so the kernels clamp what they read (ol_frontend_run).
static int ol_check_map(const char* who, const int32_t* src, const float* fill, int64_t rows) {
    if (!src && !fill) return 0;
    if (!src || !fill) return ol_fail(CP_ERR_ARG, who, "map_src and map_fill go together (both NULL: the identity)");
    if ((uintptr_t)src % 4 || (uintptr_t)fill % 4) return ol_fail(CP_ERR_ARG, who, "misaligned map");
    hipPointerAttribute_t as{}, af{};
    if (hipPointerGetAttributes(&as, src) != hipSuccess || hipPointerGetAttributes(&af, fill) != hipSuccess ||
        as.type == hipMemoryTypeUnregistered || af.type == hipMemoryTypeUnregistered) {
        (void)hipGetLastError();
        return ol_fail(CP_ERR_ARG, who, "the map must lie in memory the device reads (device or pinned host memory)");
    }
    if (as.type == hipMemoryTypeHost)
        for (int64_t i = 0; i < rows * OL_C; ++i)
            if (src[i] < -1 || src[i] >= OL_C) return ol_fail(CP_ERR_ARG, who, "map_src outside -1..11");
    if (af.type == hipMemoryTypeHost)
        for (int64_t i = 0; i < rows * OL_C; ++i)
            if (!std::isfinite(fill[i])) return ol_fail(CP_ERR_ARG, who, "map_fill must be finite");
    return 0;
}

// ---------------------------------------------------------------------------------------
// pieces of the launch chains
// ---------------------------------------------------------------------------------------
// what every front end takes from the configuration: the IIR normalised to a[0] == 1, phase and gain
static OlFrontArgs ol_front_args(const cp_online_config* c) {
    OlFrontArgs fa{};
    fa.n_coef = c->n_coef; fa.phase = c->phase; fa.gain = 1024.f;            // code/load.py:105, 2**10
    for (int i = 0; i < c->n_coef; ++i) { fa.b[i] = c->b[i] / c->a[0]; fa.a[i] = c->a[i] / c->a[0]; }
    return fa;
}

struct OlMap {                           // an electrode map as the entries take it: one row per stream, or none (the identity)
    const int32_t* src;
    const float* fill;
    float* emb;                          // rides along to the tail: where a push leaves z / |z| of its rows, (rows,16); NULL: nowhere
    const void* bank;                    // rides along to the multi-stream tail: the streams' own projections (olp_check_bank); NULL: none
};

static int ol_launch_frontend(const cp_online_config* c, OlState* state, float* X, const float* raw, int64_t n, const float* mean_std,
                              float* windows, const OlMap& map, hipStream_t st) {
    OlFrontArgs fa = ol_front_args(c);
    fa.raw = raw; fa.n = n; fa.st = state; fa.X = X; fa.windows = windows; fa.mean_std = mean_std;
    fa.map_src = map.src; fa.map_fill = map.fill;
    if (c->n_coef == 9) hipLaunchKernelGGL((ol_frontend_kernel<9>), dim3(1), dim3(256), 0, st, fa);
    else hipLaunchKernelGGL((ol_frontend_kernel<0>), dim3(1), dim3(256), 0, st, fa);
    CKL("ol_frontend_kernel");
    return 0;
}

static int olm_launch_frontend(const cp_online_config* c, int n_streams, unsigned char* base, const OlWS& w, const float* raw,
                               const int32_t* counts, int64_t total, int rows, const float* mean_std, float* windows, const OlMap& map,
                               hipStream_t st) {
    OlmFrontArgs fa{};
    fa.f = ol_front_args(c);
    fa.f.raw = raw; fa.f.X = (float*)(base + w.X); fa.f.windows = windows; fa.f.mean_std = mean_std;
    fa.f.map_src = map.src; fa.f.map_fill = map.fill;
    fa.states = (OlState*)(base + w.state); fa.meta = (OlmMeta*)(base + w.meta); fa.counts = counts; fa.total_samples = total;
    fa.rows = rows; fa.max_m = c->max_windows;
    if (c->n_coef == 9) hipLaunchKernelGGL((olm_frontend_kernel<9>), dim3(n_streams), dim3(256), 0, st, fa);
    else hipLaunchKernelGGL((olm_frontend_kernel<0>), dim3(n_streams), dim3(256), 0, st, fa);
    CKL("olm_frontend_kernel");
    return 0;
}

// The arguments of layer i of the stored model, reading `in` and writing `out`.  i = 0: conv1 + conv2 over the windows `in`
// (folded form only); 1..7: fc1..fc7, folded or unfolded; OL_PROJ: the projection as the tails and ole_accumulate take it
constexpr int OL_PROJ = CP_N_FC + 1;
static OlLayerArgs ol_layer_args(unsigned char* base, const OlWS& w, int i, const OlState* st, const void* in, void* out) {
    OlLayerArgs l{};
    l.st = st; l.out = out;
    if (i == 0) {
        l.x = (const float*)in; l.c1w = (const float*)(base + w.c1w); l.c1b = (const float*)(base + w.c1b);
        l.w = base + w.c2w; l.bias = (const float*)(base + w.c2b); l.K = OL_CONV_K; l.F = 64; l.ldo = 768; l.out_pos = 64;
    } else if (i < OL_PROJ) {
        l.act = in; l.w = base + w.fcw[i - 1]; l.bias = (const float*)(base + w.fcb[i - 1]); l.K = fcK(i - 1); l.F = 512; l.ldo = 512;
    } else {
        l.act = in; l.w = base + w.pw; l.bias = (const float*)(base + w.pb); l.K = 512; l.F = CP_D_E;
    }
    return l;
}

// The folded encoder over the windows x: conv2 into h0, then fc1..fc7, h0 -> h1 -> h0 ...: fc7 leaves its output in h1.
// launch(args, conv) enqueues one layer; conv is std::true_type for conv2
template <typename Launch>
static int ol_folded_chain(unsigned char* base, const OlWS& w, const OlState* st, const float* x, unsigned char* h0, unsigned char* h1,
                           Launch launch) {
    if (int e = launch(ol_layer_args(base, w, 0, st, x, h0), std::true_type())) return e;
    for (int i = 0; i < CP_N_FC; ++i)
        if (int e = launch(ol_layer_args(base, w, i + 1, st, i % 2 == 0 ? h0 : h1, i % 2 == 0 ? h1 : h0), std::false_type())) return e;
    return 0;
}

template <typename T>
static int ol_launch_tail(T, const cp_online_config* c, unsigned char* base, const OlWS& w, int32_t* pred, int32_t* voted, float* logits,
                          float* emb, hipStream_t st) {
    OlTailArgs ta{};
    ta.st = (OlState*)(base + w.state);
    ta.proj = ol_layer_args(base, w, OL_PROJ, ta.st, base + w.H1, nullptr);
    ta.vote = c->vote; ta.pred = pred; ta.voted = voted; ta.logits = logits; ta.emb = emb;
    hipLaunchKernelGGL((ol_tail_kernel<T>), dim3(1), dim3(OL_THREADS), 0, st, ta);
    CKL("ol_tail_kernel");
    return 0;
}

// slot 0 of a projection bank (csrc/online_projections.cuh) in compute type T
template <typename T>
static OlpSlot olp_slot0(T, const void* bank) {
    const unsigned char* b = (const unsigned char*)bank;
    return OlpSlot{b, (const float*)(b + (size_t)OLF_W * sizeof(T)), (const unsigned*)(b + (size_t)OLF_W * sizeof(T) + CP_D_E * 4)};
}

// bank: NULL, or the streams' own projections: workgroup s then takes slot s where it is set
template <typename T>
static int olm_launch_tail(T t, const cp_online_config* c, int n_streams, unsigned char* base, const OlWS& w, int32_t* pred, int32_t* voted,
                           float* logits, float* emb, const void* bank, hipStream_t st) {
    OlmTailArgs ta{};
    ta.proj = ol_layer_args(base, w, OL_PROJ, nullptr, base + w.H1, nullptr);
    ta.states = (OlState*)(base + w.state); ta.meta = (const OlmMeta*)(base + w.meta);
    ta.vote = c->vote; ta.pred = pred; ta.voted = voted; ta.logits = logits; ta.emb = emb;
    if (bank) {
        hipLaunchKernelGGL((olp_tail_kernel<T>), dim3(n_streams), dim3(OL_THREADS), 0, st, ta, olp_slot0(t, bank));
        CKL("olp_tail_kernel");
        return 0;
    }
    hipLaunchKernelGGL((olm_tail_kernel<T>), dim3(n_streams), dim3(OL_THREADS), 0, st, ta);
    CKL("olm_tail_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// online grasp decoding (csrc/online.cuh): per-stream state, folded weights and activations in the caller's workspace
// ---------------------------------------------------------------------------------------
extern "C" size_t cp_online_workspace_bytes(int32_t max_windows_per_push, int32_t dtype) {
    if (max_windows_per_push < 1) max_windows_per_push = 1;
    return ol_carve(max_windows_per_push, dtype, 1, false, false).total;
}

template <typename T>
static int online_prepare_t(T, const cp_params* p, const cp_bn_buffers* bn, float eps, unsigned char* base, const OlWS& w, hipStream_t st) {
    OlFoldArgs f{};
    f.eps = eps;
    auto set_bn = [&](int l) { f.g = p->bn_g[l]; f.beta = p->bn_b[l]; f.mean = bn->running_mean[l]; f.var = bn->running_var[l]; };
    set_bn(0);                                            // BN1 -> conv2 (and conv1 copied as it is)
    f.W = p->conv2_w; f.b = p->conv2_b; f.Wd = base + w.c2w; f.bd = (float*)(base + w.c2b); f.K = OL_CONV_K; f.mode = 2;
    f.c1w_src = p->conv1_w; f.c1b_src = p->conv1_b; f.c1w = (float*)(base + w.c1w); f.c1b = (float*)(base + w.c1b);
    hipLaunchKernelGGL((ol_fold_kernel<T>), dim3(64), dim3(256), 0, st, f);
    CKL("ol_fold_kernel");
    for (int i = 0; i < CP_N_FC; ++i) {                   // BN(i+1) -> fc(i+1); fc1's columns to the position-major layout
        set_bn(i + 1);
        f.W = p->fc_w[i]; f.b = p->fc_b[i]; f.Wd = base + w.fcw[i]; f.bd = (float*)(base + w.fcb[i]); f.K = fcK(i); f.mode = i == 0 ? 1 : 0;
        hipLaunchKernelGGL((ol_fold_kernel<T>), dim3(512), dim3(256), 0, st, f);
        CKL("ol_fold_kernel");
    }
    set_bn(CP_N_BN - 1);                                  // BN9 -> projection, which gains a bias
    f.W = p->last_w; f.b = nullptr; f.Wd = base + w.pw; f.bd = (float*)(base + w.pb); f.K = 512; f.mode = 0;
    hipLaunchKernelGGL((ol_fold_kernel<T>), dim3(CP_D_E), dim3(256), 0, st, f);
    CKL("ol_fold_kernel");
    return 0;
}

extern "C" int cp_online_prepare(const cp_online_config* cfg, const cp_params* p, const cp_bn_buffers* bn, float bn_eps, void* ws,
                                 size_t ws_bytes, void* stream) {
    OlWS w;
    if (int e = ol_check(cfg, ws, ws_bytes, false, &w)) return e;
    if (int e = ol_check_params("cp_online_prepare", p, bn, true)) return e;
    return ol_dispatch(cfg->dtype, [&](auto t) { return online_prepare_t(t, p, bn, bn_eps, (unsigned char*)ws, w, (hipStream_t)stream); });
}

extern "C" int cp_online_set_classes(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* table, const int32_t* ids,
                                     int32_t n_classes, void* stream) {
    OlWS w;
    if (int e = ol_check(cfg, ws, ws_bytes, false, &w)) return e;
    if (!table || !ids || n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return fail(CP_ERR_ARG, "cp_online_set_classes: 1..64 classes");
    hipLaunchKernelGGL(ol_set_classes_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OlState*)((unsigned char*)ws + w.state), table,
                       ids, (int)n_classes);
    CKL("ol_set_classes_kernel");
    return 0;
}

extern "C" int cp_online_reset(const cp_online_config* cfg, void* ws, size_t ws_bytes, void* stream) {
    OlWS w;
    if (int e = ol_check(cfg, ws, ws_bytes, false, &w)) return e;
    CK(hipMemsetAsync((unsigned char*)ws + w.state, 0, offsetof(OlState, K), (hipStream_t)stream));
    return 0;
}

template <typename T>
static int online_push_t(T t, const cp_online_config* c, unsigned char* base, const OlWS& w, const float* raw, int64_t n,
                         const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, const OlMap& map,
                         hipStream_t st) {
    OlState* state = (OlState*)(base + w.state);
    if (int e = ol_launch_frontend(c, state, (float*)(base + w.X), raw, n, mean_std, windows, map, st)) return e;
    auto layer = [&](const OlLayerArgs& la, auto conv) {
        constexpr bool CONV = decltype(conv)::value;
        hipLaunchKernelGGL((ol_layer_kernel<T, CONV>), CONV ? dim3(4, OL_C) : dim3(512 / 16), dim3(OL_THREADS), 0, st, la);
        CKL(CONV ? "ol_layer_kernel<conv>" : "ol_layer_kernel<fc>");
        return 0;
    };
    if (int e = ol_folded_chain(base, w, state, (const float*)(base + w.X), base + w.H0, base + w.H1, layer)) return e;
    return ol_launch_tail(t, c, base, w, pred, voted, logits, map.emb, st);
}

// cp_online_push, cp_online_adapt_push and their mapped forms
template <typename T>
static int online_adapt_push_t(T t, const cp_online_config* c, unsigned char* base, const OlWS& w, const float* raw, int64_t n,
                               const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, const OlMap& map,
                               hipStream_t st);

static int ol_push(const char* who, bool adaptive, const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw,
                   int64_t n_samples, const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows,
                   const OlMap& map, void* stream) {
    OlWS w;
    if (int e = ol_check(cfg, ws, ws_bytes, adaptive, &w)) return e;
    if (int e = ol_check_push(who, cfg, n_samples, raw, mean_std, pred, voted)) return e;
    if (int e = ol_check_map(who, map.src, map.fill, 1)) return e;
    if ((uintptr_t)map.emb % 4) return ol_fail(CP_ERR_ARG, who, "misaligned embeddings");
    if (n_samples == 0) return 0;
    return ol_dispatch(cfg->dtype, [&](auto t) {
        return adaptive ? online_adapt_push_t(t, cfg, (unsigned char*)ws, w, raw, n_samples, mean_std, pred, voted, logits, windows, map,
                                              (hipStream_t)stream)
                        : online_push_t(t, cfg, (unsigned char*)ws, w, raw, n_samples, mean_std, pred, voted, logits, windows, map,
                                        (hipStream_t)stream);
    });
}

extern "C" int cp_online_push(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                              const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, void* stream) {
    return ol_push("cp_online_push", false, cfg, ws, ws_bytes, raw, n_samples, mean_std, pred, voted, logits, windows, OlMap{}, stream);
}

extern "C" int cp_online_push_mapped(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                                     const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                     int32_t* voted, float* logits, float* windows, void* stream) {
    return ol_push("cp_online_push_mapped", false, cfg, ws, ws_bytes, raw, n_samples, mean_std, pred, voted, logits, windows,
                   OlMap{map_src, map_fill}, stream);
}

// the mapped push that also leaves z / |z| of every window in embeddings (n_windows,16); map and embeddings may be NULL
extern "C" int cp_online_push_embed(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                                    const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                    int32_t* voted, float* logits, float* windows, float* embeddings, void* stream) {
    return ol_push("cp_online_push_embed", false, cfg, ws, ws_bytes, raw, n_samples, mean_std, pred, voted, logits, windows,
                   OlMap{map_src, map_fill, embeddings}, stream);
}

// ---------------------------------------------------------------------------------------
// adaptive online decoding (csrc/online_adapt.cuh): BatchNorm unfolded, float64 statistics per stream in the workspace
// ---------------------------------------------------------------------------------------
extern "C" size_t cp_online_adapt_workspace_bytes(int32_t max_windows_per_push, int32_t dtype) {
    if (max_windows_per_push < 1) max_windows_per_push = 1;
    return ol_carve(max_windows_per_push, dtype, 1, true, false).total;
}

// BatchNorm l of the stream whose view w is
static OlaBn ola_bn(unsigned char* base, const OlWS& w, int l, int mode, double* acc, int first, int last) {
    OlaBn b{};
    b.stats = (double*)(base + w.stats) + (size_t)l * 2 * OLA_F;
    b.acc = acc ? acc + (size_t)l * 3 * OLA_F : nullptr;
    b.gamma = (const float*)(base + w.gb) + (size_t)l * 2 * OLA_F;
    b.beta = b.gamma + OLA_F;
    b.head = (const OlaHead*)(base + w.head);
    b.mode = mode; b.first = first; b.last = last;
    return b;
}

// the unfolded weights of conv2, fc1..fc7 and the projection (zero bias) into the workspace, in the layouts the folded form uses
template <typename T>
static int ola_copy_weights(T, const cp_params* p, unsigned char* base, const OlWS& w, hipStream_t st) {
    OlaCopyArgs f{};
    f.W = p->conv2_w; f.b = p->conv2_b; f.Wd = base + w.c2w; f.bd = (float*)(base + w.c2b); f.K = OL_CONV_K; f.mode = 2;
    hipLaunchKernelGGL((ola_copy_kernel<T>), dim3(64), dim3(256), 0, st, f);
    CKL("ola_copy_kernel");
    for (int i = 0; i < CP_N_FC; ++i) {
        f.W = p->fc_w[i]; f.b = p->fc_b[i]; f.Wd = base + w.fcw[i]; f.bd = (float*)(base + w.fcb[i]); f.K = fcK(i); f.mode = i == 0 ? 1 : 0;
        hipLaunchKernelGGL((ola_copy_kernel<T>), dim3(512), dim3(256), 0, st, f);
        CKL("ola_copy_kernel");
    }
    f.W = p->last_w; f.b = nullptr; f.Wd = base + w.pw; f.bd = (float*)(base + w.pb); f.K = 512; f.mode = 0;
    hipLaunchKernelGGL((ola_copy_kernel<T>), dim3(CP_D_E), dim3(256), 0, st, f);
    CKL("ola_copy_kernel");
    return 0;
}

// what both adaptive prepares hand their init kernel: gamma, beta, the running statistics if there are any, conv1 and where they go
template <typename InitArgs>
static void ola_init_args(InitArgs& ia, const cp_params* p, const cp_bn_buffers* bn, float eps, unsigned char* base, const OlWS& w) {
    for (int l = 0; l < CP_N_BN; ++l) {
        ia.g[l] = p->bn_g[l]; ia.beta[l] = p->bn_b[l];
        ia.mean[l] = bn ? bn->running_mean[l] : nullptr; ia.var[l] = bn ? bn->running_var[l] : nullptr;
    }
    ia.c1w = p->conv1_w; ia.c1b = p->conv1_b; ia.gb = (float*)(base + w.gb); ia.stats = (double*)(base + w.stats);
    ia.c1w_d = (float*)(base + w.c1w); ia.c1b_d = (float*)(base + w.c1b);
    ia.eps = eps;
}

extern "C" int cp_online_adapt_prepare(const cp_online_config* cfg, const cp_params* p, const cp_bn_buffers* bn, float bn_eps,
                                       double alpha, void* ws, size_t ws_bytes, void* stream) {
    if (!(alpha >= 0.0 && alpha < 1.0)) return fail(CP_ERR_ARG, "cp_online_adapt_prepare: alpha outside [0, 1)");
    if (!(bn_eps > 0.f)) return fail(CP_ERR_ARG, "cp_online_adapt_prepare: bn_eps must be positive");
    OlWS w;
    if (int e = ol_check(cfg, ws, ws_bytes, true, &w)) return e;
    if (int e = ol_check_params("cp_online_adapt_prepare", p, bn, false)) return e;
    unsigned char* base = (unsigned char*)ws;
    OlaBnInitArgs ia{};
    ola_init_args(ia, p, bn, bn_eps, base, w);
    ia.head = (OlaHead*)(base + w.head); ia.alpha = alpha;
    hipLaunchKernelGGL(ola_bn_init_kernel, dim3(CP_N_BN), dim3(512), 0, (hipStream_t)stream, ia);
    CKL("ola_bn_init_kernel");
    return ol_dispatch(cfg->dtype, [&](auto t) { return ola_copy_weights(t, p, base, w, (hipStream_t)stream); });
}

// conv2 GEMM: row-tile groups per feature tile for `rows` rows
static int ola_conv2_groups(int64_t rows) {
    const int64_t tiles = (rows + 15) / 16;
    return (int)(tiles < 16 ? tiles : 16);
}

// BN1 -> conv2 -> BN2 for M windows (m_fixed < 0: the push's count; max_rows bounds the row-tile groups)
template <typename T>
static int ola_conv_chain(T, unsigned char* base, const OlWS& w, const OlState* state, const float* x, int m_fixed, int64_t max_rows,
                          void* c1, float* r2, void* out, const OlaBn& bn1, const OlaBn& bn2, hipStream_t st) {
    OlaConvBnArgs cb{};
    cb.x = x; cb.c1w = (const float*)(base + w.c1w); cb.c1b = (const float*)(base + w.c1b); cb.out = c1; cb.st = state;
    cb.m_fixed = m_fixed; cb.conv1 = 1; cb.bn = bn1;
    hipLaunchKernelGGL((ola_conv_bn_kernel<T>), dim3(1), dim3(64), 0, st, cb);
    CKL("ola_conv_bn_kernel<BN1>");
    OlaGemmArgs g{};
    g.l.act = c1; g.l.w = base + w.c2w; g.l.bias = (const float*)(base + w.c2b); g.l.out = r2; g.l.st = state; g.l.K = OL_CONV_K;
    g.l.F = 64; g.l.ldo = 64; g.m_fixed = m_fixed; g.rows_per_window = OL_C;
    hipLaunchKernelGGL((ola_gemm_kernel<T>), dim3(64 / 16, ola_conv2_groups(max_rows * OL_C)), dim3(OL_THREADS), 0, st, g);
    CKL("ola_gemm_kernel");
    cb.pre = r2; cb.out = out; cb.conv1 = 0; cb.bn = bn2;
    hipLaunchKernelGGL((ola_conv_bn_kernel<T>), dim3(1), dim3(64), 0, st, cb);
    CKL("ola_conv_bn_kernel<BN2>");
    return 0;
}

// fc layer i: act [M][K] -> out [M][512] (normalised; nothing under OLA_ACC)
template <typename T>
static int ola_fc(T, unsigned char* base, const OlWS& w, const OlState* state, int i, const void* act, void* out, int m_fixed,
                  const OlaBn& bn, hipStream_t st) {
    OlaGemmArgs g{};
    g.l = ol_layer_args(base, w, i + 1, state, act, out);
    g.m_fixed = m_fixed; g.rows_per_window = 1; g.bn = bn;
    hipLaunchKernelGGL((ola_fc_kernel<T>), dim3(512 / 16), dim3(OL_THREADS), 0, st, g);
    CKL("ola_fc_kernel");
    return 0;
}

// The unfolded encoder over the windows x with every BatchNorm in `mode` (OLA_TRACK: a push; OLA_FROZEN: enrolment):
// BN1 -> conv2 -> BN2 into h0, then fc1..fc7, h0 -> h1 -> h0 ...: fc7 leaves its output in h1
template <typename T>
static int ola_chain(T t, unsigned char* base, const OlWS& w, const float* x, int m_fixed, int64_t max_rows, int mode, unsigned char* c1,
                     unsigned char* r2, unsigned char* h0, unsigned char* h1, hipStream_t st) {
    const OlState* state = (const OlState*)(base + w.state);
    auto bn = [&](int l) { return ola_bn(base, w, l, mode, nullptr, 0, 0); };
    if (int e = ola_conv_chain(t, base, w, state, x, m_fixed, max_rows, c1, (float*)r2, h0, bn(0), bn(1), st)) return e;
    for (int i = 0; i < CP_N_FC; ++i)
        if (int e = ola_fc(t, base, w, state, i, i % 2 == 0 ? h0 : h1, i % 2 == 0 ? h1 : h0, m_fixed, bn(i + 2), st)) return e;
    return 0;
}

template <typename T>
static int online_adapt_push_t(T t, const cp_online_config* c, unsigned char* base, const OlWS& w, const float* raw, int64_t n,
                               const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, const OlMap& map,
                               hipStream_t st) {
    if (int e = ol_launch_frontend(c, (OlState*)(base + w.state), (float*)(base + w.X), raw, n, mean_std, windows, map, st)) return e;
    if (int e = ola_chain(t, base, w, (const float*)(base + w.X), -1, c->max_windows, OLA_TRACK, base + w.C1, base + w.R2, base + w.H0,
                          base + w.H1, st))
        return e;
    return ol_launch_tail(t, c, base, w, pred, voted, logits, map.emb, st);
}

extern "C" int cp_online_adapt_push(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                                    const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, void* stream) {
    return ol_push("cp_online_adapt_push", true, cfg, ws, ws_bytes, raw, n_samples, mean_std, pred, voted, logits, windows, OlMap{}, stream);
}

extern "C" int cp_online_adapt_push_mapped(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                                           const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                           int32_t* voted, float* logits, float* windows, void* stream) {
    return ol_push("cp_online_adapt_push_mapped", true, cfg, ws, ws_bytes, raw, n_samples, mean_std, pred, voted, logits, windows,
                   OlMap{map_src, map_fill}, stream);
}

extern "C" int cp_online_adapt_push_embed(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                                          const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                          int32_t* voted, float* logits, float* windows, float* embeddings, void* stream) {
    return ol_push("cp_online_adapt_push_embed", true, cfg, ws, ws_bytes, raw, n_samples, mean_std, pred, voted, logits, windows,
                   OlMap{map_src, map_fill, embeddings}, stream);
}

// calibration scratch: the normalised activations of all windows (two buffers), one chunk of conv2 operand and output, and
// the float64 accumulators
struct OlaCalib {
    size_t A0, A1, C1, R2, acc, total;
};
static OlaCalib ola_calib_carve(int64_t n_windows, int dtype) {
    const size_t es = dtype == CP_BF16 ? 2 : 4;
    OlaCalib c{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    c.A0 = take((size_t)n_windows * 768 * es);
    c.A1 = take((size_t)n_windows * 512 * es);
    c.C1 = take((size_t)OL_MAXM * OL_C * OL_CONV_K * es);
    c.R2 = take((size_t)OL_MAXM * OL_C * 64 * 4);
    c.acc = take((size_t)CP_N_BN * 3 * OLA_F * 8);
    c.total = o;
    return c;
}

extern "C" size_t cp_online_adapt_calibrate_scratch_bytes(int64_t n_windows, int32_t dtype) {
    if (n_windows < 1) n_windows = 1;
    return ola_calib_carve(n_windows, dtype).total;
}

template <typename T>
static int online_adapt_calibrate_t(T t, unsigned char* base, const OlWS& w, const float* x, int64_t N, unsigned char* sc,
                                    const OlaCalib& k, hipStream_t st) {
    const OlState* state = (const OlState*)(base + w.state);
    const size_t es = sizeof(T);
    double* acc = (double*)(sc + k.acc);
    const int64_t nch = (N + OL_MAXM - 1) / OL_MAXM;
    auto rows_of = [&](int64_t ci) { return (int)(ci + 1 < nch ? OL_MAXM : N - ci * OL_MAXM); };
    // BN1: conv1 of all windows, one launch
    OlaConvBnArgs cb{};
    cb.x = x; cb.c1w = (const float*)(base + w.c1w); cb.c1b = (const float*)(base + w.c1b); cb.st = state;
    cb.m_fixed = (int)N; cb.conv1 = 1; cb.bn = ola_bn(base, w, 0, OLA_ACC, acc, 1, 1);
    hipLaunchKernelGGL((ola_conv_bn_kernel<T>), dim3(1), dim3(64), 0, st, cb);
    CKL("ola_conv_bn_kernel<BN1>");
    // BN2: per chunk BN1 (frozen) -> conv2 -> accumulate; then again with BN2 frozen into A0
    const OlaBn bn1 = ola_bn(base, w, 0, OLA_FROZEN, nullptr, 0, 0);
    for (int pass = 0; pass < 2; ++pass)
        for (int64_t ci = 0; ci < nch; ++ci) {
            const OlaBn bn2 = pass == 0 ? ola_bn(base, w, 1, OLA_ACC, acc, ci == 0, ci + 1 == nch) : ola_bn(base, w, 1, OLA_FROZEN, nullptr, 0, 0);
            if (int e = ola_conv_chain(t, base, w, state, x + ci * OL_MAXM * OL_C, rows_of(ci), OL_MAXM, sc + k.C1, (float*)(sc + k.R2),
                                       sc + k.A0 + (size_t)ci * OL_MAXM * 768 * es, bn1, bn2, st))
                return e;
        }
    // fc1..fc7: accumulate over the chunks, then (but for fc7) normalise them into the other buffer
    for (int i = 0; i < CP_N_FC; ++i) {
        const int K = fcK(i);
        unsigned char* in = sc + (i % 2 == 0 ? k.A0 : k.A1);
        unsigned char* out = sc + (i % 2 == 0 ? k.A1 : k.A0);
        for (int pass = 0; pass < (i + 1 < CP_N_FC ? 2 : 1); ++pass)
            for (int64_t ci = 0; ci < nch; ++ci) {
                const OlaBn bn = pass == 0 ? ola_bn(base, w, i + 2, OLA_ACC, acc, ci == 0, ci + 1 == nch)
                                           : ola_bn(base, w, i + 2, OLA_FROZEN, nullptr, 0, 0);
                if (int e = ola_fc(t, base, w, state, i, in + (size_t)ci * OL_MAXM * K * es, out + (size_t)ci * OL_MAXM * 512 * es,
                                   rows_of(ci), bn, st))
                    return e;
            }
    }
    return 0;
}

// both calibrate entries: check_ws(&w) checks the entry's workspace arguments and gives the view of the stream to calibrate
template <typename CheckWs>
static int ola_calibrate(const char* who, const cp_online_config* cfg, CheckWs check_ws, void* ws, const float* windows, int64_t n_windows,
                         void* scratch, size_t scratch_bytes, void* stream) {
    if (n_windows < 2) return ol_fail(CP_ERR_ARG, who, "calibration takes at least 2 windows");
    if (n_windows > (int64_t)1 << 24) return ol_fail(CP_ERR_ARG, who, "at most 2**24 windows");
    OlWS w;
    if (int e = check_ws(&w)) return e;
    if (!windows || !scratch) return ol_fail(CP_ERR_ARG, who, "windows and scratch are required");
    if ((uintptr_t)windows % 4 || (uintptr_t)scratch % 256) return ol_fail(CP_ERR_ARG, who, "misaligned input or scratch");
    const OlaCalib k = ola_calib_carve(n_windows, cfg->dtype);
    if (scratch_bytes < k.total) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    return ol_dispatch(cfg->dtype, [&](auto t) {
        return online_adapt_calibrate_t(t, (unsigned char*)ws, w, windows, n_windows, (unsigned char*)scratch, k, (hipStream_t)stream);
    });
}

extern "C" int cp_online_adapt_calibrate(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows,
                                         int64_t n_windows, void* scratch, size_t scratch_bytes, void* stream) {
    return ola_calibrate("cp_online_adapt_calibrate", cfg, [&](OlWS* w) { return ol_check(cfg, ws, ws_bytes, true, w); }, ws, windows,
                         n_windows, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_adapt_statistics(const cp_online_config* cfg, void* ws, size_t ws_bytes, double* out, void* stream) {
    OlWS w;
    if (int e = ol_check(cfg, ws, ws_bytes, true, &w)) return e;
    if (!out) return fail(CP_ERR_ARG, "cp_online_adapt_statistics: out is required");
    CK(hipMemcpyAsync(out, (unsigned char*)ws + w.stats, (size_t)OLAM_STATS * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// multi-stream online decoding (csrc/online_multi.cuh): S states, the folded weights once, rows of all streams packed
// ---------------------------------------------------------------------------------------
extern "C" size_t cp_online_multi_workspace_bytes(int32_t n_streams, int32_t max_rows, int32_t dtype) {
    if (n_streams < 1) n_streams = 1;
    if (max_rows < 1) max_rows = 1;
    return ol_carve(max_rows, dtype, n_streams, false, true).total;
}

extern "C" int cp_online_multi_prepare(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, const cp_params* p,
                                       const cp_bn_buffers* bn, float bn_eps, void* ws, size_t ws_bytes, void* stream) {
    OlWS w;
    if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, false, &w)) return e;
    if (int e = ol_check_params("cp_online_multi_prepare", p, bn, true)) return e;
    return ol_dispatch(cfg->dtype, [&](auto t) { return online_prepare_t(t, p, bn, bn_eps, (unsigned char*)ws, w, (hipStream_t)stream); });
}

extern "C" int cp_online_multi_set_classes(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                           int32_t index, const float* table, const int32_t* ids, int32_t n_classes, void* stream) {
    OlWS w;
    if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, false, &w)) return e;
    if (int e = ol_check_index("cp_online_multi_set_classes", index, n_streams)) return e;
    if (!table || !ids || n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return fail(CP_ERR_ARG, "cp_online_multi_set_classes: 1..64 classes");
    OlState* states = (OlState*)((unsigned char*)ws + w.state);
    hipLaunchKernelGGL(ol_set_classes_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, states + index, table, ids, (int)n_classes);
    CKL("ol_set_classes_kernel");
    return 0;
}

extern "C" int cp_online_multi_reset(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                     int32_t index, void* stream) {
    OlWS w;
    if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, false, &w)) return e;
    if (index < -1 || index >= n_streams) return fail(CP_ERR_ARG, "cp_online_multi_reset: stream index outside -1..n_streams-1");
    OlState* states = (OlState*)((unsigned char*)ws + w.state);
    hipLaunchKernelGGL(olm_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(256), 0, (hipStream_t)stream, states, index < 0 ? 0 : index);
    CKL("olm_reset_kernel");
    return 0;
}

// row blocks of an encoder launch with `ftiles` workgroups per row block: about OLM_TARGET_WG workgroups when there are rows
static void olm_row_blocks(int rows, int ftiles, int* blocks, int* tiles_per_block) {
    const int tiles = (rows + 15) / 16;
    int b = (OLM_TARGET_WG + ftiles - 1) / ftiles;
    if (b > tiles) b = tiles;
    *tiles_per_block = (tiles + b - 1) / b;
    *blocks = (tiles + *tiles_per_block - 1) / *tiles_per_block;
}

template <typename T>
static int online_multi_push_t(T t, const cp_online_config* c, int n_streams, unsigned char* base, const OlWS& w, const float* raw,
                               const int32_t* counts, int64_t total, int rows, const float* mean_std, int32_t* pred,
                               int32_t* voted, float* logits, float* windows, const OlMap& map, hipStream_t st) {
    if (int e = olm_launch_frontend(c, n_streams, base, w, raw, counts, total, rows, mean_std, windows, map, st)) return e;
    OlmLayerArgs la{};
    la.rows = rows;
    auto layer = [&](const OlLayerArgs& l, auto conv) {
        constexpr bool CONV = decltype(conv)::value;
        int blocks;
        olm_row_blocks(rows, CONV ? 4 * OL_C : 512 / 16, &blocks, &la.tiles_per_block);
        la.l = l;
        hipLaunchKernelGGL((olm_layer_kernel<T, CONV>), CONV ? dim3(4, OL_C, blocks) : dim3(512 / 16, blocks), dim3(OL_THREADS), 0, st, la);
        CKL(CONV ? "olm_layer_kernel<conv>" : "olm_layer_kernel<fc>");
        return 0;
    };
    if (rows > 0)
        if (int e = ol_folded_chain(base, w, nullptr, (const float*)(base + w.X), base + w.H0, base + w.H1, layer)) return e;
    return olm_launch_tail(t, c, n_streams, base, w, pred, voted, logits, map.emb, map.bank, st);
}

// cp_online_multi_push, cp_online_multi_adapt_push and their mapped forms
template <typename T>
static int online_multi_adapt_push_t(T t, const cp_online_config* c, int n_streams, unsigned char* base, const OlWS& w, const float* raw,
                                     const int32_t* counts, int64_t total, int rows, const float* mean_std, int32_t* pred,
                                     int32_t* voted, float* logits, float* windows, const OlMap& map, hipStream_t st);

static int olm_push(const char* who, bool adaptive, const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                    size_t ws_bytes, const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                    const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, const OlMap& map, void* stream) {
    OlWS w;
    if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, adaptive, &w)) return e;
    if (int e = olm_check_push(who, max_rows, raw, counts, total_samples, total_windows, mean_std, pred, voted)) return e;
    if (int e = ol_check_map(who, map.src, map.fill, n_streams)) return e;
    if ((uintptr_t)map.emb % 4) return ol_fail(CP_ERR_ARG, who, "misaligned embeddings");
    if (total_samples == 0) return 0;
    return ol_dispatch(cfg->dtype, [&](auto t) {
        return adaptive ? online_multi_adapt_push_t(t, cfg, n_streams, (unsigned char*)ws, w, raw, counts, total_samples, total_windows,
                                                    mean_std, pred, voted, logits, windows, map, (hipStream_t)stream)
                        : online_multi_push_t(t, cfg, n_streams, (unsigned char*)ws, w, raw, counts, total_samples, total_windows,
                                              mean_std, pred, voted, logits, windows, map, (hipStream_t)stream);
    });
}

extern "C" int cp_online_multi_push(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                    const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                    const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, void* stream) {
    return olm_push("cp_online_multi_push", false, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples, total_windows,
                    mean_std, pred, voted, logits, windows, OlMap{}, stream);
}

extern "C" int cp_online_multi_push_mapped(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                           const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                           const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                           int32_t* voted, float* logits, float* windows, void* stream) {
    return olm_push("cp_online_multi_push_mapped", false, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples,
                    total_windows, mean_std, pred, voted, logits, windows, OlMap{map_src, map_fill}, stream);
}

extern "C" int cp_online_multi_push_embed(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                          const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                          const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                          int32_t* voted, float* logits, float* windows, float* embeddings, void* stream) {
    return olm_push("cp_online_multi_push_embed", false, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples,
                    total_windows, mean_std, pred, voted, logits, windows, OlMap{map_src, map_fill, embeddings}, stream);
}

// ---------------------------------------------------------------------------------------
// adaptive multi-stream online decoding (csrc/online_multi_adapt.cuh): the unfolded weights once; per stream its OlState, head
// and float64 statistics; rows of all streams packed.  The workspace begins as the folded multi-stream one (n_streams states,
// then their OlmMeta), so cp_online_multi_set_classes and cp_online_multi_reset take it
// ---------------------------------------------------------------------------------------
extern "C" size_t cp_online_multi_adapt_workspace_bytes(int32_t n_streams, int32_t max_rows, int32_t dtype) {
    if (n_streams < 1) n_streams = 1;
    if (max_rows < 1) max_rows = 1;
    return ol_carve(max_rows, dtype, n_streams, true, true).total;
}

extern "C" int cp_online_multi_adapt_prepare(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, const cp_params* p,
                                             const cp_bn_buffers* bn, float bn_eps, const double* alpha, void* ws, size_t ws_bytes,
                                             void* stream) {
    if (!(bn_eps > 0.f)) return fail(CP_ERR_ARG, "cp_online_multi_adapt_prepare: bn_eps must be positive");
    OlWS w;
    if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, true, &w)) return e;
    for (int s = 0; alpha && s < n_streams; ++s)
        if (!(alpha[s] >= 0.0 && alpha[s] < 1.0)) return fail(CP_ERR_ARG, "cp_online_multi_adapt_prepare: alpha outside [0, 1)");
    if (int e = ol_check_params("cp_online_multi_adapt_prepare", p, bn, false)) return e;
    unsigned char* base = (unsigned char*)ws;
    OlamInitArgs ia{};
    ola_init_args(ia, p, bn, bn_eps, base, w);
    ia.heads = (OlaHead*)(base + w.head); ia.first = 0; ia.zero = 0; ia.set_alpha = alpha != nullptr;
    for (int s = 0; alpha && s < n_streams; ++s) ia.alpha[s] = alpha[s];
    hipLaunchKernelGGL(olam_init_kernel, dim3(CP_N_BN, n_streams), dim3(512), 0, (hipStream_t)stream, ia);
    CKL("olam_init_kernel");
    return ol_dispatch(cfg->dtype, [&](auto t) { return ola_copy_weights(t, p, base, w, (hipStream_t)stream); });
}

extern "C" int cp_online_multi_adapt_set_alpha(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                               size_t ws_bytes, int32_t index, double alpha, void* stream) {
    OlWS w;
    if (int e = olam_check_stream("cp_online_multi_adapt_set_alpha", cfg, n_streams, max_rows, ws, ws_bytes, index, &w)) return e;
    if (!(alpha >= 0.0 && alpha < 1.0)) return fail(CP_ERR_ARG, "cp_online_multi_adapt_set_alpha: alpha outside [0, 1)");
    hipLaunchKernelGGL(olam_set_alpha_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OlaHead*)((unsigned char*)ws + w.head), alpha);
    CKL("olam_set_alpha_kernel");
    return 0;
}

extern "C" int cp_online_multi_adapt_reset_statistics(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                      size_t ws_bytes, int32_t index, const cp_bn_buffers* bn, void* stream) {
    OlWS w;                                               // stream 0's view: the kernel finds stream `first` itself
    if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, true, &w)) return e;
    if (int e = ol_check_index("cp_online_multi_adapt_reset_statistics", index, n_streams)) return e;
    OlamInitArgs ia{};
    for (int l = 0; l < CP_N_BN; ++l) {
        if (bn && (!bn->running_mean[l] || !bn->running_var[l]))
            return fail(CP_ERR_ARG, "cp_online_multi_adapt_reset_statistics: running statistics");
        ia.mean[l] = bn ? bn->running_mean[l] : nullptr; ia.var[l] = bn ? bn->running_var[l] : nullptr;
    }
    ia.stats = (double*)((unsigned char*)ws + w.stats); ia.first = index; ia.zero = bn ? 0 : 1;
    hipLaunchKernelGGL(olam_init_kernel, dim3(CP_N_BN, 1), dim3(512), 0, (hipStream_t)stream, ia);
    CKL("olam_init_kernel");
    return 0;
}

extern "C" int cp_online_multi_adapt_calibrate(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                               size_t ws_bytes, int32_t index, const float* windows, int64_t n_windows, void* scratch,
                                               size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_multi_adapt_calibrate";
    return ola_calibrate(who, cfg, [&](OlWS* w) { return olam_check_stream(who, cfg, n_streams, max_rows, ws, ws_bytes, index, w); }, ws,
                         windows, n_windows, scratch, scratch_bytes, stream);
}

// row blocks of the fc launches: about OLM_TARGET_WG workgroups of 512 / 16 feature tiles when there are rows enough
static void olam_fc_blocks(int rows, int* blocks, int* rows_per_block) {
    int b = (OLM_TARGET_WG + 512 / 16 - 1) / (512 / 16);
    if (b > rows) b = rows;
    *rows_per_block = (rows + b - 1) / b;
    *blocks = (rows + *rows_per_block - 1) / *rows_per_block;
}

template <typename T>
static int online_multi_adapt_push_t(T t, const cp_online_config* c, int n_streams, unsigned char* base, const OlWS& w, const float* raw,
                                     const int32_t* counts, int64_t total, int rows, const float* mean_std, int32_t* pred,
                                     int32_t* voted, float* logits, float* windows, const OlMap& map, hipStream_t st) {
    if (int e = olm_launch_frontend(c, n_streams, base, w, raw, counts, total, rows, mean_std, windows, map, st)) return e;
    if (rows > 0) {
        const OlmMeta* meta = (const OlmMeta*)(base + w.meta);
        auto bn = [&](int l) { return ola_bn(base, w, l, OLA_TRACK, nullptr, 0, 0); };      // stream 0's: the kernels find their stream's
        OlamConvBnArgs cb{};                              // BN1 -> conv2 -> BN2, as ola_conv_chain
        cb.meta = meta;
        cb.a.x = (const float*)(base + w.X); cb.a.c1w = (const float*)(base + w.c1w); cb.a.c1b = (const float*)(base + w.c1b);
        cb.a.out = base + w.C1; cb.a.m_fixed = 0; cb.a.conv1 = 1; cb.a.bn = bn(0);
        hipLaunchKernelGGL((olam_conv_bn_kernel<T>), dim3(n_streams), dim3(64), 0, st, cb);
        CKL("olam_conv_bn_kernel<BN1>");
        OlaGemmArgs g{};
        g.l.act = base + w.C1; g.l.w = base + w.c2w; g.l.bias = (const float*)(base + w.c2b); g.l.out = base + w.R2; g.l.K = OL_CONV_K;
        g.l.F = 64; g.l.ldo = 64; g.m_fixed = rows; g.rows_per_window = OL_C;
        int blocks, tiles_per_block;
        olm_row_blocks(rows * OL_C, 64 / 16, &blocks, &tiles_per_block);
        hipLaunchKernelGGL((ola_gemm_kernel<T>), dim3(64 / 16, blocks), dim3(OL_THREADS), 0, st, g);
        CKL("ola_gemm_kernel");
        cb.a.pre = (const float*)(base + w.R2); cb.a.out = base + w.H0; cb.a.conv1 = 0; cb.a.bn = bn(1);
        hipLaunchKernelGGL((olam_conv_bn_kernel<T>), dim3(n_streams), dim3(64), 0, st, cb);
        CKL("olam_conv_bn_kernel<BN2>");
        OlamFcArgs fc{};
        fc.meta = meta; fc.n_streams = n_streams;
        olam_fc_blocks(rows, &blocks, &fc.rows_per_block);
        for (int i = 0; i < CP_N_FC; ++i) {               // H0 -> H1 -> H0 ...: fc7 leaves its output in H1
            fc.g.l = ol_layer_args(base, w, i + 1, nullptr, base + (i % 2 == 0 ? w.H0 : w.H1), base + (i % 2 == 0 ? w.H1 : w.H0));
            fc.g.rows_per_window = 1; fc.g.bn = bn(i + 2);
            hipLaunchKernelGGL((olam_fc_kernel<T>), dim3(512 / 16, blocks), dim3(OL_THREADS), 0, st, fc);
            CKL("olam_fc_kernel");
        }
    }
    return olm_launch_tail(t, c, n_streams, base, w, pred, voted, logits, map.emb, map.bank, st);
}

extern "C" int cp_online_multi_adapt_push(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                          const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                          const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows,
                                          void* stream) {
    return olm_push("cp_online_multi_adapt_push", true, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples, total_windows,
                    mean_std, pred, voted, logits, windows, OlMap{}, stream);
}

extern "C" int cp_online_multi_adapt_push_mapped(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                 size_t ws_bytes, const float* raw, const int32_t* counts, int64_t total_samples,
                                                 int32_t total_windows, const float* mean_std, const int32_t* map_src,
                                                 const float* map_fill, int32_t* pred, int32_t* voted, float* logits, float* windows,
                                                 void* stream) {
    return olm_push("cp_online_multi_adapt_push_mapped", true, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples,
                    total_windows, mean_std, pred, voted, logits, windows, OlMap{map_src, map_fill}, stream);
}

extern "C" int cp_online_multi_adapt_push_embed(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                size_t ws_bytes, const float* raw, const int32_t* counts, int64_t total_samples,
                                                int32_t total_windows, const float* mean_std, const int32_t* map_src,
                                                const float* map_fill, int32_t* pred, int32_t* voted, float* logits, float* windows,
                                                float* embeddings, void* stream) {
    return olm_push("cp_online_multi_adapt_push_embed", true, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples,
                    total_windows, mean_std, pred, voted, logits, windows, OlMap{map_src, map_fill, embeddings}, stream);
}

extern "C" int cp_online_multi_adapt_statistics(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                size_t ws_bytes, int32_t index, double* out, void* stream) {
    OlWS w;
    if (int e = olam_check_stream("cp_online_multi_adapt_statistics", cfg, n_streams, max_rows, ws, ws_bytes, index, &w)) return e;
    if (!out) return fail(CP_ERR_ARG, "cp_online_multi_adapt_statistics: out is required");
    CK(hipMemcpyAsync(out, (unsigned char*)ws + w.stats, (size_t)OLAM_STATS * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// class enrolment (csrc/online_enroll.cuh): the front end alone, per-class sums of z / |z| in the caller's float64
// accumulator, and the blend of those directions with the rows a decoder has
// ---------------------------------------------------------------------------------------
extern "C" size_t cp_online_frontend_state_bytes(void) { return align256(offsetof(OlState, K)); }

static int ol_windows(const char* who, const cp_online_config* cfg, void* state, size_t state_bytes, const float* raw, int64_t n_samples,
                      const float* mean_std, const OlMap& map, float* windows, void* stream) {
    if (!cfg || !state) return ol_fail(CP_ERR_ARG, who, "config and state are required");
    if (int e = ol_check_config(cfg, state)) return e;
    if (state_bytes < cp_online_frontend_state_bytes()) return ol_fail(CP_ERR_ARG, who, "state too small");
    if (n_samples < 0 || n_samples > (int64_t)CP_ONLINE_STRIDE * cfg->max_windows)
        return ol_fail(CP_ERR_ARG, who, "a call takes at most 20 * max_windows samples");
    if (int e = ol_check_map(who, map.src, map.fill, 1)) return e;
    if (n_samples == 0) return 0;
    if (!raw || !mean_std || !windows) return ol_fail(CP_ERR_ARG, who, "raw, mean_std and windows are required");
    if ((uintptr_t)raw % 4 || (uintptr_t)mean_std % 4 || (uintptr_t)windows % 4) return ol_fail(CP_ERR_ARG, who, "misaligned input");
    OlFrontArgs fa = ol_front_args(cfg);
    fa.raw = raw; fa.n = n_samples; fa.st = (OlState*)state; fa.X = windows; fa.windows = nullptr; fa.mean_std = mean_std;
    fa.map_src = map.src; fa.map_fill = map.fill;
    if (cfg->n_coef == 9) hipLaunchKernelGGL((ole_windows_kernel<9>), dim3(1), dim3(256), 0, (hipStream_t)stream, fa);
    else hipLaunchKernelGGL((ole_windows_kernel<0>), dim3(1), dim3(256), 0, (hipStream_t)stream, fa);
    CKL("ole_windows_kernel");
    return 0;
}

extern "C" int cp_online_windows(const cp_online_config* cfg, void* state, size_t state_bytes, const float* raw, int64_t n_samples,
                                 const float* mean_std, float* windows, void* stream) {
    return ol_windows("cp_online_windows", cfg, state, state_bytes, raw, n_samples, mean_std, OlMap{}, windows, stream);
}

extern "C" int cp_online_windows_mapped(const cp_online_config* cfg, void* state, size_t state_bytes, const float* raw,
                                        int64_t n_samples, const float* mean_std, const int32_t* map_src, const float* map_fill,
                                        float* windows, void* stream) {
    return ol_windows("cp_online_windows_mapped", cfg, state, state_bytes, raw, n_samples, mean_std, OlMap{map_src, map_fill}, windows,
                      stream);
}

// enrolment scratch: the activations of one chunk of <= 256 windows (the adaptive form also conv2's operand and output)
struct OleScratch {
    size_t C1, R2, H0, H1, total;
};
static OleScratch ole_carve(int64_t n_windows, int dtype) {
    const size_t es = dtype == CP_BF16 ? 2 : 4;
    const size_t rows = (size_t)(((n_windows < OL_MAXM ? n_windows : OL_MAXM) + 15) / 16 * 16);
    OleScratch c{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    c.C1 = take(rows * OL_C * OL_CONV_K * es);
    c.R2 = take(rows * OL_C * 64 * 4);
    c.H0 = take(rows * 768 * es);
    c.H1 = take(rows * 512 * es);
    c.total = o;
    return c;
}

extern "C" size_t cp_online_enroll_scratch_bytes(int64_t n_windows, int32_t dtype) {
    if (n_windows < 1) n_windows = 1;
    return ole_carve(n_windows, dtype).total;
}

// One chunk of m <= 256 windows x through the decoder's own encoder: the folded encoder as a push runs it, or (adaptive) the
// unfolded one with the statistics frozen, the OLA_FROZEN pass of online_adapt_calibrate_t.  fc7's output goes to rows 0..m-1
// of h1 (rows of 512 in the compute dtype); fc1's, fc3's and fc5's pass through the same rows
template <typename T>
static int ole_encode_chunk(T t, bool adaptive, unsigned char* base, const OlWS& w, const float* x, int m, unsigned char* sc,
                            const OleScratch& k, unsigned char* h1, hipStream_t st) {
    auto layer = [&](const OlLayerArgs& la, auto conv) {
        constexpr bool CONV = decltype(conv)::value;
        hipLaunchKernelGGL((ole_layer_kernel<T, CONV>), CONV ? dim3(4, OL_C) : dim3(512 / 16), dim3(OL_THREADS), 0, st, la, m);
        CKL(CONV ? "ole_layer_kernel<conv>" : "ole_layer_kernel<fc>");
        return 0;
    };
    return adaptive ? ola_chain(t, base, w, x, m, m, OLA_FROZEN, sc + k.C1, sc + k.R2, sc + k.H0, h1, st)
                    : ol_folded_chain(base, w, nullptr, x, sc + k.H0, h1, layer);
}

// The caller's windows through the encoder chunk by chunk, each chunk's z / |z| added to acc
template <typename T>
static int online_enroll_t(T t, bool adaptive, unsigned char* base, const OlWS& w, const float* x, int64_t N, const int32_t* slots,
                           int n_classes, double* acc, unsigned char* sc, const OleScratch& k, const OlpSlot* own, hipStream_t st) {
    for (int64_t r0 = 0; r0 < N; r0 += OL_MAXM) {
        const int m = (int)(N - r0 < OL_MAXM ? N - r0 : OL_MAXM);
        if (int e = ole_encode_chunk(t, adaptive, base, w, x + r0 * OL_C, m, sc, k, sc + k.H1, st)) return e;
        OleAccArgs a{};
        a.proj = ol_layer_args(base, w, OL_PROJ, nullptr, sc + k.H1, nullptr);
        a.slots = slots + r0; a.acc = acc; a.M = m; a.n_classes = n_classes;
        if (own) {                                        // the stream's own projection where its slot is set
            hipLaunchKernelGGL((olp_accumulate_kernel<T>), dim3(1), dim3(OL_THREADS), 0, st, a, *own);
            CKL("olp_accumulate_kernel");
            continue;
        }
        hipLaunchKernelGGL((ole_accumulate_kernel<T>), dim3(1), dim3(OL_THREADS), 0, st, a);
        CKL("ole_accumulate_kernel");
    }
    return 0;
}

// the accumulate entries: check_ws(&w) checks the entry's workspace arguments and gives the view of the stream to enrol
// with.  n_windows == 0 is a valid empty call.  own_slot (the *_proj entries): NULL, or the slot of the stream in its bank
template <typename CheckWs>
static int ole_enroll(const char* who, const cp_online_config* cfg, CheckWs check_ws, bool adaptive, void* ws, const float* windows,
                      int64_t n_windows, const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes,
                      void* stream, const void* own_slot = nullptr) {
    OlWS w;
    if (int e = check_ws(&w)) return e;
    if (n_windows < 0 || n_windows > (int64_t)1 << 24) return ol_fail(CP_ERR_ARG, who, "n_windows outside 0..2**24");
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return ol_fail(CP_ERR_ARG, who, "1..64 classes");
    if (!acc) return ol_fail(CP_ERR_ARG, who, "acc is required");
    if ((uintptr_t)acc % 8) return ol_fail(CP_ERR_ARG, who, "misaligned acc");
    if (n_windows == 0) return 0;
    if (!windows || !slots || !scratch) return ol_fail(CP_ERR_ARG, who, "windows, slots and scratch are required");
    if ((uintptr_t)windows % 4 || (uintptr_t)slots % 4 || (uintptr_t)scratch % 256) return ol_fail(CP_ERR_ARG, who, "misaligned input or scratch");
    const OleScratch k = ole_carve(n_windows, cfg->dtype);
    if (scratch_bytes < k.total) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    return ol_dispatch(cfg->dtype, [&](auto t) {
        const OlpSlot own = own_slot ? olp_slot0(t, own_slot) : OlpSlot{};
        return online_enroll_t(t, adaptive, (unsigned char*)ws, w, windows, n_windows, slots, n_classes, acc, (unsigned char*)scratch, k,
                               own_slot ? &own : nullptr, (hipStream_t)stream);
    });
}

extern "C" int cp_online_enroll(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows,
                                const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes, void* stream) {
    return ole_enroll("cp_online_enroll", cfg, [&](OlWS* w) { return ol_check(cfg, ws, ws_bytes, false, w); }, false, ws, windows,
                      n_windows, slots, n_classes, acc, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_adapt_enroll(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows,
                                      const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes,
                                      void* stream) {
    return ole_enroll("cp_online_adapt_enroll", cfg, [&](OlWS* w) { return ol_check(cfg, ws, ws_bytes, true, w); }, true, ws, windows,
                      n_windows, slots, n_classes, acc, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_multi_enroll(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                      const float* windows, int64_t n_windows, const int32_t* slots, int32_t n_classes, double* acc,
                                      void* scratch, size_t scratch_bytes, void* stream) {
    return ole_enroll("cp_online_multi_enroll", cfg, [&](OlWS* w) { return olm_check(cfg, n_streams, max_rows, ws, ws_bytes, false, w); },
                      false, ws, windows, n_windows, slots, n_classes, acc, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_multi_adapt_enroll(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                            int32_t index, const float* windows, int64_t n_windows, const int32_t* slots,
                                            int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_multi_adapt_enroll";
    return ole_enroll(who, cfg, [&](OlWS* w) { return olam_check_stream(who, cfg, n_streams, max_rows, ws, ws_bytes, index, w); }, true,
                      ws, windows, n_windows, slots, n_classes, acc, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_enroll_table(const double* acc, int32_t n_classes, const float* prior, double mix, int32_t min_windows,
                                      float* table, void* stream) {
    if (!acc || !prior || !table) return fail(CP_ERR_ARG, "cp_online_enroll_table: acc, prior and table are required");
    if ((uintptr_t)acc % 8 || (uintptr_t)prior % 4 || (uintptr_t)table % 4) return fail(CP_ERR_ARG, "cp_online_enroll_table: misaligned input");
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return fail(CP_ERR_ARG, "cp_online_enroll_table: 1..64 classes");
    if (!(mix >= 0.0 && mix <= 1.0)) return fail(CP_ERR_ARG, "cp_online_enroll_table: mix outside [0, 1]");
    if (min_windows < 1) return fail(CP_ERR_ARG, "cp_online_enroll_table: min_windows must be at least 1");
    hipLaunchKernelGGL(ole_table_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, (int)n_classes, prior, mix, (double)min_windows,
                       table);
    CKL("ole_table_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// head fine-tuning (csrc/online_finetune.cuh): the tail inputs of a labelled recording, a caller-owned state with the masters
// of the projection and the class rows, steps of two launches each, and the tail's projection written and read
// ---------------------------------------------------------------------------------------
static_assert(OLF_CHUNK == CP_ONLINE_FINETUNE_CHUNK && OLF_TRAIN_PROJ == CP_ONLINE_FINETUNE_PROJECTION &&
              OLF_TRAIN_ROWS == CP_ONLINE_FINETUNE_ROWS, "fine-tuning constants");

// The workspace checks of the entries that read or write the tail's weights.  The four forms lay their weights out at
// different offsets, and an entry cannot see which form prepared a workspace: these entries take ws_bytes as the form's own
// cp_online_*workspace_bytes and refuse any other size, so a folded entry on an adaptive workspace (or the reverse) is an error
// and not a write into the wrong block.
static int olf_check_single(const char* who, const cp_online_config* c, void* ws, size_t ws_bytes, bool adaptive, OlWS* out) {
    if (int e = ol_check(c, ws, ws_bytes, adaptive, out)) return e;
    if (ws_bytes != out->total)
        return ol_fail(CP_ERR_ARG, who, adaptive ? "ws_bytes is not cp_online_adapt_workspace_bytes: not an adaptive workspace of this configuration"
                                                 : "ws_bytes is not cp_online_workspace_bytes: not a folded workspace of this configuration");
    return 0;
}
static int olf_check_multi(const char* who, const cp_online_config* c, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                           bool adaptive, OlWS* out) {
    if (int e = olm_check(c, n_streams, max_rows, ws, ws_bytes, adaptive, out)) return e;
    if (ws_bytes != out->total) return ol_fail(CP_ERR_ARG, who, "ws_bytes is not this form's workspace size for n_streams, max_rows and dtype");
    return 0;
}

template <typename T>
static int online_tail_inputs_t(T t, bool adaptive, unsigned char* base, const OlWS& w, const float* x, int64_t N, unsigned char* out,
                                unsigned char* sc, const OleScratch& k, hipStream_t st) {
    for (int64_t r0 = 0; r0 < N; r0 += OL_MAXM) {
        const int m = (int)(N - r0 < OL_MAXM ? N - r0 : OL_MAXM);
        if (int e = ole_encode_chunk(t, adaptive, base, w, x + r0 * OL_C, m, sc, k, out + (size_t)r0 * 512 * sizeof(T), st)) return e;
    }
    return 0;
}

// the four tail-input entries: check_ws(&w) as for ole_enroll.  n_windows == 0 is a valid empty call
template <typename CheckWs>
static int olf_tail_inputs(const char* who, const cp_online_config* cfg, CheckWs check_ws, bool adaptive, void* ws, const float* windows,
                           int64_t n_windows, void* out, void* scratch, size_t scratch_bytes, void* stream) {
    OlWS w;
    if (int e = check_ws(&w)) return e;
    if (n_windows < 0 || n_windows > (int64_t)1 << 24) return ol_fail(CP_ERR_ARG, who, "n_windows outside 0..2**24");
    if (n_windows == 0) return 0;
    if (!windows || !out || !scratch) return ol_fail(CP_ERR_ARG, who, "windows, out and scratch are required");
    if ((uintptr_t)windows % 4 || (uintptr_t)out % 16 || (uintptr_t)scratch % 256) return ol_fail(CP_ERR_ARG, who, "misaligned input, out or scratch");
    const OleScratch k = ole_carve(n_windows, cfg->dtype);
    if (scratch_bytes < k.total) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    return ol_dispatch(cfg->dtype, [&](auto t) {
        return online_tail_inputs_t(t, adaptive, (unsigned char*)ws, w, windows, n_windows, (unsigned char*)out, (unsigned char*)scratch, k,
                                    (hipStream_t)stream);
    });
}

extern "C" int cp_online_tail_inputs(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows,
                                     void* out, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_tail_inputs";
    return olf_tail_inputs(who, cfg, [&](OlWS* w) { return olf_check_single(who, cfg, ws, ws_bytes, false, w); }, false, ws, windows,
                           n_windows, out, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_adapt_tail_inputs(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows,
                                           int64_t n_windows, void* out, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_adapt_tail_inputs";
    return olf_tail_inputs(who, cfg, [&](OlWS* w) { return olf_check_single(who, cfg, ws, ws_bytes, true, w); }, true, ws, windows,
                           n_windows, out, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_multi_tail_inputs(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                           const float* windows, int64_t n_windows, void* out, void* scratch, size_t scratch_bytes,
                                           void* stream) {
    const char* who = "cp_online_multi_tail_inputs";
    return olf_tail_inputs(who, cfg, [&](OlWS* w) { return olf_check_multi(who, cfg, n_streams, max_rows, ws, ws_bytes, false, w); }, false,
                           ws, windows, n_windows, out, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_multi_adapt_tail_inputs(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                 size_t ws_bytes, int32_t index, const float* windows, int64_t n_windows, void* out,
                                                 void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_multi_adapt_tail_inputs";
    auto check = [&](OlWS* w) {
        if (int e = olf_check_multi(who, cfg, n_streams, max_rows, ws, ws_bytes, true, w)) return e;
        if (int e = ol_check_index(who, index, n_streams)) return e;
        *w = ol_stream(*w, index);
        return 0;
    };
    return olf_tail_inputs(who, cfg, check, true, ws, windows, n_windows, out, scratch, scratch_bytes, stream);
}

// the state of a fine-tuning run: OlfHead, the masters theta = (W, b, E), their initial values and Adam moments (f32, OLF_P
// each), the copy of W in the compute dtype (sized for f32), the step's reduced gradient (float64), the slots and one slab per
// chunk of OLF_CHUNK windows
struct OlfState {
    size_t head, theta, theta0, m, v, wT, grad, slots, slabs, total;
};
static OlfState olf_carve(int64_t n_windows) {
    OlfState c{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    const size_t chunks = (size_t)((n_windows + OLF_CHUNK - 1) / OLF_CHUNK);
    c.head = take(sizeof(OlfHead));
    c.theta = take((size_t)OLF_P * 4);
    c.theta0 = take((size_t)OLF_P * 4);
    c.m = take((size_t)OLF_P * 4);
    c.v = take((size_t)OLF_P * 4);
    c.wT = take((size_t)OLF_W * 4);
    c.grad = take((size_t)OLF_P * 8);
    c.slots = take((size_t)n_windows * 4);
    c.slabs = take(chunks * OLF_SLAB * 4);
    c.total = o;
    return c;
}

extern "C" size_t cp_online_finetune_state_bytes(int64_t n_windows, int32_t n_classes) {
    (void)n_classes;                                         // the state holds 64 rows whatever K is
    if (n_windows < 1) n_windows = 1;
    return olf_carve(n_windows).total;
}

// what init, steps and read check alike
static int olf_check_state(const char* who, void* state, size_t state_bytes, int64_t n_windows, int32_t n_classes, OlfState* out) {
    if (!state) return ol_fail(CP_ERR_ARG, who, "state is required");
    if ((uintptr_t)state % 256) return ol_fail(CP_ERR_ARG, who, "state not 256-byte aligned");
    if (n_windows < 1 || n_windows > (int64_t)1 << 24) return ol_fail(CP_ERR_ARG, who, "n_windows outside 1..2**24");
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return ol_fail(CP_ERR_ARG, who, "1..64 classes");
    *out = olf_carve(n_windows);
    if (state_bytes < out->total) return ol_fail(CP_ERR_ARG, who, "state too small");
    return 0;
}

extern "C" int cp_online_finetune_init(void* state, size_t state_bytes, int32_t dtype, const float* W, const float* b, const float* E,
                                       const int32_t* slots, int64_t n_windows, int32_t n_classes, int32_t balanced, void* stream) {
    const char* who = "cp_online_finetune_init";
    OlfState k;
    if (int e = olf_check_state(who, state, state_bytes, n_windows, n_classes, &k)) return e;
    if (dtype != CP_F32 && dtype != CP_BF16) return ol_fail(CP_ERR_ARG, who, "dtype must be CP_F32 or CP_BF16");
    if (!W || !b || !E || !slots) return ol_fail(CP_ERR_ARG, who, "W, b, E and slots are required");
    if ((uintptr_t)W % 4 || (uintptr_t)b % 4 || (uintptr_t)E % 4 || (uintptr_t)slots % 4) return ol_fail(CP_ERR_ARG, who, "misaligned input");
    if (balanced != 0 && balanced != 1) return ol_fail(CP_ERR_ARG, who, "balanced must be 0 or 1");
    unsigned char* s = (unsigned char*)state;
    OlfInitArgs a{};
    a.head = (OlfHead*)(s + k.head); a.W = W; a.b = b; a.E = E; a.slots_in = slots;
    a.theta = (float*)(s + k.theta); a.theta0 = (float*)(s + k.theta0); a.m = (float*)(s + k.m); a.v = (float*)(s + k.v);
    a.wT = s + k.wT; a.slots = (int32_t*)(s + k.slots); a.grad = (double*)(s + k.grad);
    a.n = (int)n_windows; a.K = n_classes; a.balanced = balanced;
    return ol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((olf_init_kernel<T>), dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
        CKL("olf_init_kernel");
        return 0;
    });
}

extern "C" int cp_online_finetune_steps(const cp_online_config* cfg, void* state, size_t state_bytes, const void* u, int64_t n_windows,
                                        int32_t n_classes, int32_t n_steps, double lr, double lr_rows, double scale, double anchor,
                                        int32_t flags, double* loss_out, void* stream) {
    const char* who = "cp_online_finetune_steps";
    if (!cfg) return ol_fail(CP_ERR_ARG, who, "config is required");
    if (cfg->dtype != CP_F32 && cfg->dtype != CP_BF16) return ol_fail(CP_ERR_ARG, who, "dtype must be CP_F32 or CP_BF16 (no 8-bit path)");
    OlfState k;
    if (int e = olf_check_state(who, state, state_bytes, n_windows, n_classes, &k)) return e;
    if (n_steps < 0) return ol_fail(CP_ERR_ARG, who, "negative n_steps");
    if (!std::isfinite(lr) || !std::isfinite(lr_rows) || lr < 0.0 || lr_rows < 0.0) return ol_fail(CP_ERR_ARG, who, "lr and lr_rows must be finite and >= 0");
    if (!std::isfinite(scale) || !std::isfinite((double)(float)scale)) return ol_fail(CP_ERR_ARG, who, "scale must be finite");
    if (!std::isfinite(anchor) || anchor < 0.0) return ol_fail(CP_ERR_ARG, who, "anchor must be finite and >= 0");
    if (flags & ~(OLF_TRAIN_PROJ | OLF_TRAIN_ROWS)) return ol_fail(CP_ERR_ARG, who, "unknown flags");
    if (!u) return ol_fail(CP_ERR_ARG, who, "u is required");
    if ((uintptr_t)u % 16) return ol_fail(CP_ERR_ARG, who, "u not 16-byte aligned");
    if (n_steps == 0) return 0;
    if (!loss_out) return ol_fail(CP_ERR_ARG, who, "loss_out is required");
    if ((uintptr_t)loss_out % 8) return ol_fail(CP_ERR_ARG, who, "misaligned loss_out");
    unsigned char* s = (unsigned char*)state;
    const int chunks = (int)((n_windows + OLF_CHUNK - 1) / OLF_CHUNK);
    OlfStepArgs sa{};
    sa.proj.act = u; sa.proj.w = s + k.wT; sa.proj.bias = (const float*)(s + k.theta) + OLF_W; sa.proj.K = 512; sa.proj.F = CP_D_E;
    sa.head = (OlfHead*)(s + k.head); sa.E = (const float*)(s + k.theta) + OLF_B; sa.slots = (const int32_t*)(s + k.slots);
    sa.slabs = (float*)(s + k.slabs); sa.N = (int)n_windows; sa.K = n_classes; sa.scale = (float)scale;
    OlfUpdateArgs ua{};
    ua.head = sa.head; ua.theta = (float*)(s + k.theta); ua.m = (float*)(s + k.m); ua.v = (float*)(s + k.v);
    ua.theta0 = (const float*)(s + k.theta0); ua.wT = s + k.wT; ua.grad = (double*)(s + k.grad); ua.slabs = sa.slabs;
    ua.chunks = chunks; ua.K = n_classes; ua.flags = flags; ua.lr = lr; ua.lr_rows = lr_rows; ua.anchor = anchor;
    return ol_dispatch(cfg->dtype, [&](auto t) {
        using T = decltype(t);
        for (int i = 0; i < n_steps; ++i) {
            hipLaunchKernelGGL((olf_step_kernel<T>), dim3(chunks), dim3(OL_THREADS), 0, (hipStream_t)stream, sa);
            CKL("olf_step_kernel");
            ua.loss = loss_out + i;
            hipLaunchKernelGGL((olf_update_kernel<T>), dim3(OLF_P / OLF_UPDATE_THREADS + 1), dim3(OLF_UPDATE_THREADS), 0,
                               (hipStream_t)stream, ua);
            CKL("olf_update_kernel");
        }
        return 0;
    });
}

extern "C" int cp_online_finetune_read(void* state, size_t state_bytes, int64_t n_windows, int32_t n_classes, float* W, float* b, float* E,
                                       double* grad_out, void* stream) {
    const char* who = "cp_online_finetune_read";
    OlfState k;
    if (int e = olf_check_state(who, state, state_bytes, n_windows, n_classes, &k)) return e;
    if (!W || !b || !E) return ol_fail(CP_ERR_ARG, who, "W, b and E are required");
    if ((uintptr_t)W % 4 || (uintptr_t)b % 4 || (uintptr_t)E % 4 || (uintptr_t)grad_out % 8) return ol_fail(CP_ERR_ARG, who, "misaligned output");
    const unsigned char* s = (const unsigned char*)state;
    const float* theta = (const float*)(s + k.theta);
    hipStream_t st = (hipStream_t)stream;
    CK(hipMemcpyAsync(W, theta, (size_t)OLF_W * 4, hipMemcpyDeviceToDevice, st));
    CK(hipMemcpyAsync(b, theta + OLF_W, (size_t)CP_D_E * 4, hipMemcpyDeviceToDevice, st));
    CK(hipMemcpyAsync(E, theta + OLF_B, (size_t)n_classes * CP_D_E * 4, hipMemcpyDeviceToDevice, st));
    if (grad_out) CK(hipMemcpyAsync(grad_out, s + k.grad, (size_t)(OLF_B + n_classes * CP_D_E) * 8, hipMemcpyDeviceToDevice, st));
    return 0;
}

// the tail's projection of a workspace whose view is w: written from f32 (set) or read back widened
static int olf_projection(const char* who, const cp_online_config* cfg, void* ws, const OlWS& w, bool set, float* W, float* b, void* stream) {
    if (!W || !b) return ol_fail(CP_ERR_ARG, who, "W and b are required");
    if ((uintptr_t)W % 4 || (uintptr_t)b % 4) return ol_fail(CP_ERR_ARG, who, "misaligned W or b");
    unsigned char* base = (unsigned char*)ws;
    return ol_dispatch(cfg->dtype, [&](auto t) {
        using T = decltype(t);
        if (set) hipLaunchKernelGGL((olf_set_projection_kernel<T>), dim3(OLF_W / 256), dim3(256), 0, (hipStream_t)stream, (const float*)W,
                                    (const float*)b, (T*)(base + w.pw), (float*)(base + w.pb));
        else hipLaunchKernelGGL((olf_get_projection_kernel<T>), dim3(OLF_W / 256), dim3(256), 0, (hipStream_t)stream,
                                (const T*)(base + w.pw), (const float*)(base + w.pb), W, b);
        CKL(set ? "olf_set_projection_kernel" : "olf_get_projection_kernel");
        return 0;
    });
}

extern "C" int cp_online_set_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* W, const float* b, void* stream) {
    const char* who = "cp_online_set_projection";
    OlWS w;
    if (int e = olf_check_single(who, cfg, ws, ws_bytes, false, &w)) return e;
    return olf_projection(who, cfg, ws, w, true, (float*)W, (float*)b, stream);
}

extern "C" int cp_online_adapt_set_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* W, const float* b,
                                              void* stream) {
    const char* who = "cp_online_adapt_set_projection";
    OlWS w;
    if (int e = olf_check_single(who, cfg, ws, ws_bytes, true, &w)) return e;
    return olf_projection(who, cfg, ws, w, true, (float*)W, (float*)b, stream);
}

extern "C" int cp_online_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, float* W, float* b, void* stream) {
    const char* who = "cp_online_projection";
    OlWS w;
    if (int e = olf_check_single(who, cfg, ws, ws_bytes, false, &w)) return e;
    return olf_projection(who, cfg, ws, w, false, W, b, stream);
}

extern "C" int cp_online_adapt_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, float* W, float* b, void* stream) {
    const char* who = "cp_online_adapt_projection";
    OlWS w;
    if (int e = olf_check_single(who, cfg, ws, ws_bytes, true, &w)) return e;
    return olf_projection(who, cfg, ws, w, false, W, b, stream);
}

extern "C" int cp_online_multi_projection(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                          float* W, float* b, void* stream) {
    const char* who = "cp_online_multi_projection";
    OlWS w;
    if (int e = olf_check_multi(who, cfg, n_streams, max_rows, ws, ws_bytes, false, &w)) return e;
    return olf_projection(who, cfg, ws, w, false, W, b, stream);
}

extern "C" int cp_online_multi_adapt_projection(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                size_t ws_bytes, float* W, float* b, void* stream) {
    const char* who = "cp_online_multi_adapt_projection";
    OlWS w;
    if (int e = olf_check_multi(who, cfg, n_streams, max_rows, ws, ws_bytes, true, &w)) return e;
    return olf_projection(who, cfg, ws, w, false, W, b, stream);
}

// ---------------------------------------------------------------------------------------
// grasp command gate (csrc/online_gate.cuh): one OgState per stream in a workspace of its own, behind any decoder's logits
// ---------------------------------------------------------------------------------------
static_assert(OG_MAXK == CP_ONLINE_MAX_CLASSES && OG_MAXVOTE == CP_ONLINE_MAX_VOTE && OG_MAXM == CP_ONLINE_MAX_WINDOWS, "gate limits");
static_assert(sizeof(OgState) == 4 * (8 + 2 * OG_MAXK + 2 * OG_MAXVOTE), "OgState is 648 words (CommandGate.state reads it back)");

static int og_check(const char* who, const cp_online_gate_config* c, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!c || !ws) return bad("config and workspace are required");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if (c->vote < 1 || c->vote > CP_ONLINE_MAX_VOTE) return bad("vote outside 1..256");
    if (c->min_votes < 1) return bad("min_votes must be at least 1");
    if (c->dwell < 1) return bad("dwell must be at least 1");
    if (c->release < 0) return bad("release must not be negative");
    if (c->weight != 0 && c->weight != 1) return bad("weight must be 0 (count) or 1 (margin)");
    if (!(c->min_margin >= 0.f) || std::isinf(c->min_margin)) return bad("min_margin must be finite and >= 0");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes < (size_t)n_streams * sizeof(OgState)) return bad("workspace too small");
    return 0;
}

extern "C" size_t cp_online_gate_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(OgState));
}

extern "C" int cp_online_gate_set_classes(const cp_online_gate_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                          const int32_t* ids, const float* min_cosine, int32_t n_classes, void* stream) {
    if (int e = og_check("cp_online_gate_set_classes", cfg, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index("cp_online_gate_set_classes", index, n_streams)) return e;
    if (!ids || !min_cosine || n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES)
        return fail(CP_ERR_ARG, "cp_online_gate_set_classes: 1..64 classes, with ids and min_cosine");
    OgClassArgs c{};
    c.K = n_classes;
    for (int k = 0; k < n_classes; ++k) {
        if (ids[k] < 0 || ids[k] == INT32_MAX || (k > 0 && ids[k] <= ids[k - 1]))
            return fail(CP_ERR_ARG, "cp_online_gate_set_classes: ids must be ascending, distinct and in 0..2^31-2");
        if (std::isnan(min_cosine[k])) return fail(CP_ERR_ARG, "cp_online_gate_set_classes: min_cosine must not be NaN");
        c.ids[k] = ids[k];
        c.min_cosine[k] = min_cosine[k];
    }
    hipLaunchKernelGGL(og_set_classes_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OgState*)ws + index, c);
    CKL("og_set_classes_kernel");
    return 0;
}

extern "C" int cp_online_gate_reset(const cp_online_gate_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                    void* stream) {
    if (int e = og_check("cp_online_gate_reset", cfg, n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return fail(CP_ERR_ARG, "cp_online_gate_reset: stream index outside -1..n_streams-1");
    hipLaunchKernelGGL(og_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(64), 0, (hipStream_t)stream, (OgState*)ws,
                       index < 0 ? 0 : index);
    CKL("og_reset_kernel");
    return 0;
}

extern "C" int cp_online_gate_push(const cp_online_gate_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const float* logits,
                                   int32_t ldl, const int32_t* row0, const int32_t* m, int32_t total_rows, int32_t* command,
                                   int32_t* accepted, float* conf, float* margin, void* stream) {
    if (int e = og_check("cp_online_gate_push", cfg, n_streams, ws, ws_bytes)) return e;
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return fail(CP_ERR_ARG, "cp_online_gate_push: total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (ldl < 1) return fail(CP_ERR_ARG, "cp_online_gate_push: ldl must be at least 1");
    if (!logits || !row0 || !m || !command || !accepted)
        return fail(CP_ERR_ARG, "cp_online_gate_push: logits, row0, m, command and accepted are required");
    if ((uintptr_t)logits % 4 || (uintptr_t)row0 % 4 || (uintptr_t)m % 4 || (uintptr_t)command % 4 || (uintptr_t)accepted % 4 ||
        (uintptr_t)conf % 4 || (uintptr_t)margin % 4)
        return fail(CP_ERR_ARG, "cp_online_gate_push: misaligned argument");
    OgPushArgs a{};
    a.states = (OgState*)ws; a.logits = logits; a.row0 = row0; a.m = m; a.ldl = ldl; a.total_rows = total_rows;
    a.command = command; a.accepted = accepted; a.conf = conf; a.margin = margin;
    a.c.vote = cfg->vote; a.c.min_votes = cfg->min_votes; a.c.dwell = cfg->dwell; a.c.release = cfg->release; a.c.weight = cfg->weight;
    a.c.min_margin = cfg->min_margin;
    hipLaunchKernelGGL(og_push_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    CKL("og_push_kernel");
    return 0;
}

// gate sweep: n_configs settings over one recording, one wave each, scored on the device (og_rows_kernel, og_sweep_kernel)
static_assert(OG_SCORES == CP_ONLINE_GATE_SCORES && sizeof(OgRow) == 12, "gate sweep layout");
static_assert(sizeof(OgConfig) == sizeof(cp_online_gate_config), "the sweep reads cp_online_gate_config from the device as OgConfig");

extern "C" size_t cp_online_gate_sweep_scratch_bytes(int64_t n_rows) {
    if (n_rows < 1) n_rows = 1;
    return align256((size_t)n_rows * sizeof(OgRow));
}

extern "C" int cp_online_gate_sweep(const float* logits, int32_t ldl, int64_t n_rows, int32_t n_classes, const int32_t* expected_slot,
                                    const cp_online_gate_config* configs, const float* min_cosine, int32_t n_configs, void* scratch,
                                    size_t scratch_bytes, int64_t* scores, int32_t* commands, void* stream) {
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return fail(CP_ERR_ARG, "cp_online_gate_sweep: n_classes outside 1..64");
    if (ldl < n_classes) return fail(CP_ERR_ARG, "cp_online_gate_sweep: ldl must be at least n_classes");
    if (n_configs < 1 || n_configs > CP_ONLINE_GATE_SWEEP_MAX_CONFIGS)
        return fail(CP_ERR_ARG, "cp_online_gate_sweep: n_configs outside 1..65536");
    if (n_rows < 1 || n_rows > INT32_MAX) return fail(CP_ERR_ARG, "cp_online_gate_sweep: n_rows outside 1..2^31-1");
    if (!logits || !expected_slot || !configs || !min_cosine || !scratch || !scores)
        return fail(CP_ERR_ARG, "cp_online_gate_sweep: logits, expected_slot, configs, min_cosine, scratch and scores are required");
    if ((uintptr_t)logits % 4 || (uintptr_t)expected_slot % 4 || (uintptr_t)configs % 4 || (uintptr_t)min_cosine % 4 ||
        (uintptr_t)scratch % 4 || (uintptr_t)scores % 8 || (uintptr_t)commands % 4)
        return fail(CP_ERR_ARG, "cp_online_gate_sweep: misaligned argument");
    if (scratch_bytes < (size_t)n_rows * sizeof(OgRow)) return fail(CP_ERR_ARG, "cp_online_gate_sweep: scratch too small");
    const int rows_per_block = 4 * OG_ROWS_PER_WAVE;
    hipLaunchKernelGGL(og_rows_kernel, dim3((unsigned)((n_rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, (hipStream_t)stream,
                       logits, (int)ldl, (long long)n_rows, (int)n_classes, (OgRow*)scratch);
    CKL("og_rows_kernel");
    OgSweepArgs a{};
    a.rows = (const OgRow*)scratch; a.expected = expected_slot; a.configs = (const OgConfig*)configs; a.min_cosine = min_cosine;
    a.n_rows = n_rows; a.n_configs = n_configs; a.K = n_classes; a.scores = (long long*)scores; a.commands = commands;
    hipLaunchKernelGGL(og_sweep_kernel, dim3((n_configs + OG_SWEEP_WAVES - 1) / OG_SWEEP_WAVES), dim3(64 * OG_SWEEP_WAVES), 0,
                       (hipStream_t)stream, a);
    CKL("og_sweep_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// grasp sequence decoder (csrc/online_sequence.cuh): one SqState per stream in a workspace of its own, behind any decoder's logits
// ---------------------------------------------------------------------------------------
static_assert(SQ_MAXK == CP_ONLINE_MAX_CLASSES && SQ_MAXM == CP_ONLINE_MAX_WINDOWS && SQ_RING == CP_ONLINE_SEQ_RING, "sequence limits");
static_assert(SQ_COST_MAX == CP_ONLINE_SEQ_MAX_COST && SQ_FLOOR == CP_ONLINE_SEQ_FLOOR, "sequence constants");
static_assert(sizeof(SqState) == 4 * (8 + 4 * SQ_MAXK + SQ_MAXK * SQ_MAXK + SQ_MAXK) + SQ_RING * SQ_BP_STRIDE,
              "SqState is 4424 words and 4352 ring bytes (SequenceGate.state reads it back)");
static_assert(sizeof(SqSweepConfig) == sizeof(cp_online_seq_config), "the sweep reads cp_online_seq_config from the device as SqSweepConfig");

static int sq_check(const char* who, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!ws) return bad("workspace is required");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes < (size_t)n_streams * sizeof(SqState)) return bad("workspace too small");
    return 0;
}

extern "C" size_t cp_online_seq_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(SqState));
}

extern "C" int cp_online_seq_set_model(int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, const int32_t* ids,
                                       const float* min_cosine, int32_t n_classes, const int32_t* cost, int32_t lag, void* stream) {
    if (int e = sq_check("cp_online_seq_set_model", n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index("cp_online_seq_set_model", index, n_streams)) return e;
    if (!ids || !min_cosine || n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES)
        return fail(CP_ERR_ARG, "cp_online_seq_set_model: 1..64 classes, with ids and min_cosine");
    if (!cost || (uintptr_t)cost % 4) return fail(CP_ERR_ARG, "cp_online_seq_set_model: cost is required, 4-byte aligned");
    if (lag < 0 || lag >= CP_ONLINE_SEQ_RING) return fail(CP_ERR_ARG, "cp_online_seq_set_model: lag outside 0..63");
    SqModelArgs c{};
    c.K = n_classes;
    c.lag = lag;
    for (int k = 0; k < n_classes; ++k) {
        if (ids[k] < 0 || ids[k] == INT32_MAX || (k > 0 && ids[k] <= ids[k - 1]))
            return fail(CP_ERR_ARG, "cp_online_seq_set_model: ids must be ascending, distinct and in 0..2^31-2");
        if (std::isnan(min_cosine[k])) return fail(CP_ERR_ARG, "cp_online_seq_set_model: min_cosine must not be NaN");
        c.ids[k] = ids[k];
        c.thr[k] = (int)std::nearbyint(std::fmin(std::fmax(min_cosine[k], -2.0f), 2.0f) * SQ_SCALE);     // q(): half-even, exact product
    }
    hipLaunchKernelGGL(seq_set_model_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (SqState*)ws + index, c, cost);
    CKL("seq_set_model_kernel");
    return 0;
}

extern "C" int cp_online_seq_reset(int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream) {
    if (int e = sq_check("cp_online_seq_reset", n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return fail(CP_ERR_ARG, "cp_online_seq_reset: stream index outside -1..n_streams-1");
    hipLaunchKernelGGL(seq_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(64), 0, (hipStream_t)stream, (SqState*)ws,
                       index < 0 ? 0 : index);
    CKL("seq_reset_kernel");
    return 0;
}

extern "C" int cp_online_seq_push(int32_t n_streams, void* ws, size_t ws_bytes, const float* logits, int32_t ldl, const int32_t* row0,
                                  const int32_t* m, int32_t total_rows, int32_t* command, int32_t* now, int32_t* lead, void* stream) {
    if (int e = sq_check("cp_online_seq_push", n_streams, ws, ws_bytes)) return e;
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return fail(CP_ERR_ARG, "cp_online_seq_push: total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (ldl < 1) return fail(CP_ERR_ARG, "cp_online_seq_push: ldl must be at least 1");
    if (!logits || !row0 || !m || !command) return fail(CP_ERR_ARG, "cp_online_seq_push: logits, row0, m and command are required");
    if ((uintptr_t)logits % 4 || (uintptr_t)row0 % 4 || (uintptr_t)m % 4 || (uintptr_t)command % 4 || (uintptr_t)now % 4 ||
        (uintptr_t)lead % 4)
        return fail(CP_ERR_ARG, "cp_online_seq_push: misaligned argument");
    SqPushArgs a{};
    a.states = (SqState*)ws; a.logits = logits; a.row0 = row0; a.m = m; a.ldl = ldl; a.total_rows = total_rows;
    a.command = command; a.now = now; a.lead = lead;
    hipLaunchKernelGGL(seq_push_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    CKL("seq_push_kernel");
    return 0;
}

// sequence sweep: n_configs (model, lag, thresholds) over one recording, one wave each, scored on the device
extern "C" size_t cp_online_seq_sweep_scratch_bytes(int64_t n_rows) {
    if (n_rows < 1) n_rows = 1;
    return align256((size_t)n_rows * SQ_MAXK * sizeof(int32_t));
}

extern "C" int cp_online_seq_sweep(const float* logits, int32_t ldl, int64_t n_rows, int32_t n_classes, const int32_t* expected_slot,
                                   const int32_t* costs, int32_t n_models, const cp_online_seq_config* configs, const float* min_cosine,
                                   int32_t n_configs, void* scratch, size_t scratch_bytes, int64_t* scores, int32_t* commands,
                                   void* stream) {
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return fail(CP_ERR_ARG, "cp_online_seq_sweep: n_classes outside 1..64");
    if (ldl < n_classes) return fail(CP_ERR_ARG, "cp_online_seq_sweep: ldl must be at least n_classes");
    if (n_configs < 1 || n_configs > CP_ONLINE_SEQ_SWEEP_MAX_CONFIGS)
        return fail(CP_ERR_ARG, "cp_online_seq_sweep: n_configs outside 1..65536");
    if (n_models < 1 || n_models > CP_ONLINE_SEQ_SWEEP_MAX_CONFIGS)
        return fail(CP_ERR_ARG, "cp_online_seq_sweep: n_models outside 1..65536");
    if (n_rows < 1 || n_rows > INT32_MAX) return fail(CP_ERR_ARG, "cp_online_seq_sweep: n_rows outside 1..2^31-1");
    if (!logits || !expected_slot || !costs || !configs || !min_cosine || !scratch || !scores)
        return fail(CP_ERR_ARG, "cp_online_seq_sweep: logits, expected_slot, costs, configs, min_cosine, scratch and scores are required");
    if ((uintptr_t)logits % 4 || (uintptr_t)expected_slot % 4 || (uintptr_t)costs % 4 || (uintptr_t)configs % 4 ||
        (uintptr_t)min_cosine % 4 || (uintptr_t)scratch % 4 || (uintptr_t)scores % 8 || (uintptr_t)commands % 4)
        return fail(CP_ERR_ARG, "cp_online_seq_sweep: misaligned argument");
    if (scratch_bytes < (size_t)n_rows * SQ_MAXK * sizeof(int32_t)) return fail(CP_ERR_ARG, "cp_online_seq_sweep: scratch too small");
    const int rows_per_block = 4 * SQ_ROWS_PER_WAVE;
    hipLaunchKernelGGL(seq_rows_kernel, dim3((unsigned)((n_rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, (hipStream_t)stream,
                       logits, (int)ldl, (long long)n_rows, (int)n_classes, (int32_t*)scratch);
    CKL("seq_rows_kernel");
    SqSweepArgs a{};
    a.q = (const int32_t*)scratch; a.expected = expected_slot; a.costs = costs; a.configs = (const SqSweepConfig*)configs;
    a.min_cosine = min_cosine; a.n_rows = n_rows; a.n_models = n_models; a.n_configs = n_configs; a.K = n_classes;
    a.scores = (long long*)scores; a.commands = commands;
    hipLaunchKernelGGL(seq_sweep_kernel, dim3((n_configs + SQ_SWEEP_WAVES - 1) / SQ_SWEEP_WAVES), dim3(64 * SQ_SWEEP_WAVES), 0,
                       (hipStream_t)stream, a);
    CKL("seq_sweep_kernel");
    return 0;
}

// grasp-set search: n_subsets class subsets over one cued recording, one wave each, scored on the device (csrc/online_subsets.cuh)
static_assert(OS_SCORES == CP_ONLINE_SUBSET_SCORES && OS_ORDER == CP_ONLINE_MAX_CLASSES, "subset sweep layout");

extern "C" size_t cp_online_subset_sweep_scratch_bytes(int64_t n_rows) {
    if (n_rows < 1) n_rows = 1;
    return align256((size_t)n_rows * OS_ORDER);
}

extern "C" int cp_online_subset_sweep(const float* logits, int32_t ldl, int64_t n_rows, int32_t n_classes, const int32_t* expected_slot,
                                      const uint64_t* subsets, int32_t n_subsets, int32_t vote, void* scratch, size_t scratch_bytes,
                                      int64_t* scores, int32_t* class_hits, void* stream) {
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return fail(CP_ERR_ARG, "cp_online_subset_sweep: n_classes outside 1..64");
    if (ldl < n_classes) return fail(CP_ERR_ARG, "cp_online_subset_sweep: ldl must be at least n_classes");
    if (n_subsets < 1 || n_subsets > CP_ONLINE_SUBSET_SWEEP_MAX_SUBSETS)
        return fail(CP_ERR_ARG, "cp_online_subset_sweep: n_subsets outside 1..1048576");
    if (vote < 1 || vote > CP_ONLINE_MAX_VOTE) return fail(CP_ERR_ARG, "cp_online_subset_sweep: vote outside 1..256");
    if (n_rows < 1 || n_rows > INT32_MAX) return fail(CP_ERR_ARG, "cp_online_subset_sweep: n_rows outside 1..2^31-1");
    if (!logits || !expected_slot || !subsets || !scratch || !scores)
        return fail(CP_ERR_ARG, "cp_online_subset_sweep: logits, expected_slot, subsets, scratch and scores are required");
    if ((uintptr_t)logits % 4 || (uintptr_t)expected_slot % 4 || (uintptr_t)subsets % 8 || (uintptr_t)scratch % 16 ||
        (uintptr_t)scores % 8 || (uintptr_t)class_hits % 4)
        return fail(CP_ERR_ARG, "cp_online_subset_sweep: misaligned argument");
    if (scratch_bytes < (size_t)n_rows * OS_ORDER) return fail(CP_ERR_ARG, "cp_online_subset_sweep: scratch too small");
    hipLaunchKernelGGL(os_rows_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, (int)ldl,
                       (long long)n_rows, (int)n_classes, (unsigned char*)scratch);
    CKL("os_rows_kernel");
    OsSweepArgs a{};
    a.order = (const unsigned char*)scratch; a.expected = expected_slot; a.subsets = (const unsigned long long*)subsets;
    a.n_rows = n_rows; a.n_subsets = n_subsets; a.K = n_classes; a.vote = vote; a.scores = (long long*)scores; a.class_hits = class_hits;
    hipLaunchKernelGGL(os_sweep_kernel, dim3((n_subsets + OS_WAVES - 1) / OS_WAVES), dim3(64 * OS_WAVES), 0, (hipStream_t)stream, a);
    CKL("os_sweep_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// grasp drive (csrc/online_drive.cuh): one OdState per stream in a workspace of its own, behind any decoder's windows and the
// class the hand follows
// ---------------------------------------------------------------------------------------
static_assert(OD_MAXK == CP_ONLINE_MAX_CLASSES && OD_MAXSMOOTH == CP_ONLINE_DRIVE_MAX_SMOOTH && OD_MAXM == CP_ONLINE_MAX_WINDOWS &&
              OD_ONE == CP_ONLINE_DRIVE_ONE && OD_C == CP_EMG_DIM, "drive limits");
static_assert(sizeof(OdState) == 4 * (8 + 16 + OD_MAXK + 48 + OD_MAXK * OD_C + OD_MAXK * OD_C / 4 + OD_MAXSMOOTH),
              "OdState is 1352 words (GraspDrive.state reads it back)");
static_assert(sizeof(OdConfig) == sizeof(cp_online_drive_config) && sizeof(OdProfileArgs) <= 4096, "drive arguments");

static int od_check(const char* who, const cp_online_drive_config* c, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!c || !ws) return bad("config and workspace are required");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if (c->smooth < 1 || c->smooth > CP_ONLINE_DRIVE_MAX_SMOOTH) return bad("smooth outside 1..256");
    if (c->on_level < 0 || c->on_level > CP_ONLINE_DRIVE_ONE) return bad("on_level outside 0..4096");
    if (c->off_level < 0 || c->off_level > CP_ONLINE_DRIVE_ONE) return bad("off_level outside 0..4096");
    if (c->off_level > c->on_level) return bad("off_level must not exceed on_level");
    if (c->rise < 1 || c->rise > CP_ONLINE_DRIVE_ONE) return bad("rise outside 1..4096");
    if (c->fall < 1 || c->fall > CP_ONLINE_DRIVE_ONE) return bad("fall outside 1..4096");
    if (c->bad_after < 1 || c->bad_after > 65535) return bad("bad_after outside 1..65535");
    if (c->good_after < 1 || c->good_after > 65535) return bad("good_after outside 1..65535");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes < (size_t)n_streams * sizeof(OdState)) return bad("workspace too small");
    return 0;
}

static OdConfig od_config(const cp_online_drive_config* c) {
    OdConfig o;
    o.smooth = c->smooth; o.on_level = c->on_level; o.off_level = c->off_level; o.rise = c->rise; o.fall = c->fall;
    o.bad_after = c->bad_after; o.good_after = c->good_after;
    return o;
}

extern "C" size_t cp_online_drive_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(OdState));
}

extern "C" int cp_online_drive_set_profile(const cp_online_drive_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                           const int32_t* ids, int32_t n_classes, const float* rest, const float* span,
                                           const int32_t* weight, const float* low, const float* high, void* stream) {
    const char* who = "cp_online_drive_set_profile";
    if (int e = od_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if (!ids || !rest || !span || !weight || !low || !high || n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES)
        return ol_fail(CP_ERR_ARG, who, "1..64 classes, with ids, rest, span, weight, low and high");
    for (int k = 0; k < n_classes; ++k)
        if (ids[k] < 0 || ids[k] == INT32_MAX || (k > 0 && ids[k] <= ids[k - 1]))
            return ol_fail(CP_ERR_ARG, who, "ids must be ascending, distinct and in 0..2^31-2");
    for (int c = 0; c < OD_C; ++c) {
        if (!std::isfinite(rest[c])) return ol_fail(CP_ERR_ARG, who, "rest must be finite");
        if (std::isnan(low[c]) || std::isnan(high[c]) || low[c] > high[c]) return ol_fail(CP_ERR_ARG, who, "low and high must not be NaN, low <= high");
    }
    for (int i = 0; i < n_classes * OD_C; ++i)
        if (weight[i] < 0 || weight[i] > 255) return ol_fail(CP_ERR_ARG, who, "weight outside 0..255");
    OdProfileArgs p{};
    p.K = n_classes;
    for (int k = 0; k < n_classes; ++k) p.ids[k] = ids[k];
    for (int c = 0; c < OD_C; ++c) {
        p.par[c] = rest[c];
        p.par[16 + c] = low[c];
        p.par[32 + c] = high[c];
    }
    for (int first = 0; first < OD_MAXK; first += OD_PROFILE_SLOTS) {
        p.first = first;
        for (int i = 0; i < OD_PROFILE_SLOTS * OD_C; ++i) {
            const bool on = first * OD_C + i < n_classes * OD_C;
            p.span[i] = on ? span[first * OD_C + i] : 0.f;
            p.weight[i] = on ? (unsigned char)weight[first * OD_C + i] : (unsigned char)0;
        }
        hipLaunchKernelGGL(od_set_profile_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OdState*)ws + index, p);
        CKL("od_set_profile_kernel");
    }
    return 0;
}

extern "C" int cp_online_drive_reset(const cp_online_drive_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                     void* stream) {
    if (int e = od_check("cp_online_drive_reset", cfg, n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return fail(CP_ERR_ARG, "cp_online_drive_reset: stream index outside -1..n_streams-1");
    hipLaunchKernelGGL(od_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(64), 0, (hipStream_t)stream, (OdState*)ws,
                       index < 0 ? 0 : index);
    CKL("od_reset_kernel");
    return 0;
}

extern "C" int cp_online_drive_push(const cp_online_drive_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const float* windows,
                                    int32_t ldw, const int32_t* cls, const int32_t* row0, const int32_t* m, int32_t total_rows,
                                    float* drive, int32_t* active, int32_t* bad, void* stream) {
    if (int e = od_check("cp_online_drive_push", cfg, n_streams, ws, ws_bytes)) return e;
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return fail(CP_ERR_ARG, "cp_online_drive_push: total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (ldw < CP_EMG_DIM) return fail(CP_ERR_ARG, "cp_online_drive_push: ldw must be at least 12");
    if (!windows || !cls || !row0 || !m || !drive || !active || !bad)
        return fail(CP_ERR_ARG, "cp_online_drive_push: windows, cls, row0, m, drive, active and bad are required");
    if ((uintptr_t)windows % 4 || (uintptr_t)cls % 4 || (uintptr_t)row0 % 4 || (uintptr_t)m % 4 || (uintptr_t)drive % 4 ||
        (uintptr_t)active % 4 || (uintptr_t)bad % 4)
        return fail(CP_ERR_ARG, "cp_online_drive_push: misaligned argument");
    OdPushArgs a{};
    a.states = (OdState*)ws; a.windows = windows; a.cls = cls; a.row0 = row0; a.m = m; a.ldw = ldw; a.total_rows = total_rows;
    a.drive = drive; a.active = active; a.bad = bad; a.c = od_config(cfg);
    hipLaunchKernelGGL(od_push_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    CKL("od_push_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// electrode-map sweep (csrc/online_maps.cuh): n_maps maps over one cued recording's RMS series, rows (map, window) through the
// decoder's own encoder in chunks that fill the chip, then one wave per map through the vote ring
// ---------------------------------------------------------------------------------------
static_assert(OLMAP_SCORES == CP_ONLINE_MAP_SCORES, "map sweep layout");
constexpr int64_t OLMAP_DEFAULT_CHUNK = 16384;           // rows: 1024 tiles, two per workgroup slot of a 512-workgroup fc launch x 32

// sweep scratch: the windows and activations of one chunk (the adaptive forms also conv2's operand and output for a piece of
// <= 256 rows)
struct OlMapScratch {
    size_t X, C1, R2, H0, H1, total;
    int64_t chunk;
};
static OlMapScratch olmap_carve(int64_t n_rows, int64_t chunk_rows, int dtype, bool adaptive) {
    const size_t es = dtype == CP_BF16 ? 2 : 4;
    if (n_rows < 1) n_rows = 1;
    int64_t chunk = chunk_rows > 0 ? chunk_rows : OLMAP_DEFAULT_CHUNK;
    if (chunk > CP_ONLINE_MULTI_MAX_ROWS) chunk = CP_ONLINE_MULTI_MAX_ROWS;
    if (chunk > n_rows) chunk = n_rows;
    const size_t R = (size_t)((chunk + 15) / 16 * 16);
    OlMapScratch c{};
    c.chunk = chunk;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    c.X = take(R * OL_C * 4);
    if (adaptive) {
        c.C1 = take((size_t)OL_MAXM * OL_C * OL_CONV_K * es);
        c.R2 = take((size_t)OL_MAXM * OL_C * 64 * 4);
    }
    c.H0 = take(R * 768 * es);
    c.H1 = take(R * 512 * es);
    c.total = o;
    return c;
}

extern "C" size_t cp_online_map_sweep_scratch_bytes(int64_t n_rows, int64_t chunk_rows, int32_t dtype, int32_t adaptive) {
    return olmap_carve(n_rows, chunk_rows, dtype, adaptive != 0).total;
}

struct OlMapSweep {                      // what the four sweep entries share
    const float* rms;                    // (M, 12) device
    int64_t n_windows;
    const float* mean_std;
    const int32_t* map_src;              // (n_maps, 12)
    const float* map_fill;
    int32_t n_maps, n_classes;
    const int32_t* expected_slot;        // (M) device
    int64_t chunk_rows;
    void* scratch;
    size_t scratch_bytes;
    int32_t *pred, *voted;               // (n_maps, M)
    int64_t* scores;
    int32_t* class_hits;
    const void* own_slot;                // (the *_proj entries) NULL, or the slot of the stream in its projection bank
};

template <typename T>
static int online_map_sweep_t(T t, bool adaptive, const cp_online_config* c, unsigned char* base, const OlWS& w, const OlMapSweep& a,
                              const OlMapScratch& k, hipStream_t st) {
    unsigned char* sc = (unsigned char*)a.scratch;
    const size_t es = sizeof(T);
    const OlState* state = (const OlState*)(base + w.state);
    const int M = (int)a.n_windows;
    const int64_t total = (int64_t)a.n_maps * M;
    for (int64_t r0 = 0; r0 < total; r0 += k.chunk) {
        const int rows = (int)(total - r0 < k.chunk ? total - r0 : k.chunk);
        OlMapBuildArgs b{};
        b.R = a.rms; b.mean_std = a.mean_std; b.src = a.map_src; b.fill = a.map_fill; b.X = (float*)(sc + k.X); b.row0 = r0; b.rows = rows;
        b.M = M;
        hipLaunchKernelGGL(olmap_build_kernel, dim3((unsigned)(((int64_t)rows * OL_C + 255) / 256)), dim3(256), 0, st, b);
        CKL("olmap_build_kernel");
        if (adaptive) {
            for (int p0 = 0; p0 < rows; p0 += OL_MAXM) {
                const int m = rows - p0 < OL_MAXM ? rows - p0 : OL_MAXM;
                if (int e = ola_chain(t, base, w, (const float*)(sc + k.X) + (size_t)p0 * OL_C, m, m, OLA_FROZEN, sc + k.C1, sc + k.R2,
                                      sc + k.H0 + (size_t)p0 * 768 * es, sc + k.H1 + (size_t)p0 * 512 * es, st))
                    return e;
            }
        } else {
            OlmLayerArgs la{};
            la.rows = rows;
            auto layer = [&](const OlLayerArgs& l, auto conv) {
                constexpr bool CONV = decltype(conv)::value;
                int blocks;
                olm_row_blocks(rows, CONV ? 4 * OL_C : 512 / 16, &blocks, &la.tiles_per_block);
                la.l = l;
                hipLaunchKernelGGL((olm_layer_kernel<T, CONV>), CONV ? dim3(4, OL_C, blocks) : dim3(512 / 16, blocks), dim3(OL_THREADS), 0, st,
                                   la);
                CKL(CONV ? "olm_layer_kernel<conv>" : "olm_layer_kernel<fc>");
                return 0;
            };
            if (int e = ol_folded_chain(base, w, nullptr, (const float*)(sc + k.X), sc + k.H0, sc + k.H1, layer)) return e;
        }
        OlMapTailArgs ta{};
        ta.proj = ol_layer_args(base, w, OL_PROJ, nullptr, sc + k.H1, nullptr);
        ta.st = state; ta.slot = a.pred + r0; ta.rows = rows;
        int blocks;
        olm_row_blocks(rows, 1, &blocks, &ta.tiles_per_block);
        if (a.own_slot) {
            hipLaunchKernelGGL((olp_map_tail_kernel<T>), dim3(blocks), dim3(OL_THREADS), 0, st, ta, olp_slot0(t, a.own_slot));
            CKL("olp_map_tail_kernel");
            continue;
        }
        hipLaunchKernelGGL((olmap_tail_kernel<T>), dim3(blocks), dim3(OL_THREADS), 0, st, ta);
        CKL("olmap_tail_kernel");
    }
    OlMapVoteArgs v{};
    v.st = state; v.expected = a.expected_slot; v.pred = a.pred; v.voted = a.voted; v.scores = (long long*)a.scores;
    v.class_hits = a.class_hits; v.n_maps = a.n_maps; v.M = M; v.vote = c->vote;
    hipLaunchKernelGGL(olmap_vote_kernel, dim3((a.n_maps + OLMAP_WAVES - 1) / OLMAP_WAVES), dim3(64 * OLMAP_WAVES), 0, st, v);
    CKL("olmap_vote_kernel");
    return 0;
}

// the four sweep entries: check_ws(&w) checks the entry's workspace arguments and gives the view of the stream to sweep with
template <typename CheckWs>
static int olmap_sweep(const char* who, const cp_online_config* cfg, CheckWs check_ws, bool adaptive, void* ws, const OlMapSweep& a,
                       void* stream) {
    if (a.n_maps < 1 || a.n_maps > CP_ONLINE_MAP_SWEEP_MAX_MAPS) return ol_fail(CP_ERR_ARG, who, "n_maps outside 1..65536");
    if (a.n_classes < 1 || a.n_classes > CP_ONLINE_MAX_CLASSES) return ol_fail(CP_ERR_ARG, who, "n_classes outside 1..64");
    if (a.n_windows < 1 || (int64_t)a.n_maps * a.n_windows > INT32_MAX) return ol_fail(CP_ERR_ARG, who, "n_windows < 1, or n_maps * n_windows >= 2^31");
    if (a.chunk_rows < 0) return ol_fail(CP_ERR_ARG, who, "chunk_rows must not be negative (0: the default)");
    OlWS w;
    if (int e = check_ws(&w)) return e;
    if (!a.rms || !a.mean_std || !a.map_src || !a.map_fill || !a.expected_slot || !a.scratch || !a.pred || !a.scores)
        return ol_fail(CP_ERR_ARG, who, "rms, mean_std, map_src, map_fill, expected_slot, scratch, pred and scores are required");
    if ((uintptr_t)a.rms % 4 || (uintptr_t)a.mean_std % 4 || (uintptr_t)a.expected_slot % 4 || (uintptr_t)a.scratch % 256 ||
        (uintptr_t)a.pred % 4 || (uintptr_t)a.voted % 4 || (uintptr_t)a.scores % 8 || (uintptr_t)a.class_hits % 4)
        return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    if (int e = ol_check_map(who, a.map_src, a.map_fill, a.n_maps)) return e;
    const OlMapScratch k = olmap_carve((int64_t)a.n_maps * a.n_windows, a.chunk_rows, cfg->dtype, adaptive);
    if (a.scratch_bytes < k.total) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    return ol_dispatch(cfg->dtype, [&](auto t) {
        return online_map_sweep_t(t, adaptive, cfg, (unsigned char*)ws, w, a, k, (hipStream_t)stream);
    });
}

extern "C" int cp_online_map_sweep(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* rms, int64_t n_windows,
                                   const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps,
                                   int32_t n_classes, const int32_t* expected_slot, int64_t chunk_rows, void* scratch,
                                   size_t scratch_bytes, int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits,
                                   void* stream) {
    const OlMapSweep a{rms, n_windows, mean_std, map_src, map_fill, n_maps, n_classes, expected_slot, chunk_rows, scratch, scratch_bytes,
                       pred, voted, scores, class_hits};
    return olmap_sweep("cp_online_map_sweep", cfg, [&](OlWS* w) { return ol_check(cfg, ws, ws_bytes, false, w); }, false, ws, a, stream);
}

extern "C" int cp_online_adapt_map_sweep(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* rms, int64_t n_windows,
                                         const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps,
                                         int32_t n_classes, const int32_t* expected_slot, int64_t chunk_rows, void* scratch,
                                         size_t scratch_bytes, int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits,
                                         void* stream) {
    const OlMapSweep a{rms, n_windows, mean_std, map_src, map_fill, n_maps, n_classes, expected_slot, chunk_rows, scratch, scratch_bytes,
                       pred, voted, scores, class_hits};
    return olmap_sweep("cp_online_adapt_map_sweep", cfg, [&](OlWS* w) { return ol_check(cfg, ws, ws_bytes, true, w); }, true, ws, a, stream);
}

extern "C" int cp_online_multi_map_sweep(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                         int32_t index, const float* rms, int64_t n_windows, const float* mean_std,
                                         const int32_t* map_src, const float* map_fill, int32_t n_maps, int32_t n_classes,
                                         const int32_t* expected_slot, int64_t chunk_rows, void* scratch, size_t scratch_bytes,
                                         int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits, void* stream) {
    const char* who = "cp_online_multi_map_sweep";
    const OlMapSweep a{rms, n_windows, mean_std, map_src, map_fill, n_maps, n_classes, expected_slot, chunk_rows, scratch, scratch_bytes,
                       pred, voted, scores, class_hits};
    auto check_ws = [&](OlWS* w) {
        if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, false, w)) return e;
        if (int e = ol_check_index(who, index, n_streams)) return e;
        w->state += (size_t)index * sizeof(OlState);       // the stream's class table; the folded weights are shared
        return 0;
    };
    return olmap_sweep(who, cfg, check_ws, false, ws, a, stream);
}

extern "C" int cp_online_multi_adapt_map_sweep(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                               size_t ws_bytes, int32_t index, const float* rms, int64_t n_windows,
                                               const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps,
                                               int32_t n_classes, const int32_t* expected_slot, int64_t chunk_rows, void* scratch,
                                               size_t scratch_bytes, int32_t* pred, int32_t* voted, int64_t* scores,
                                               int32_t* class_hits, void* stream) {
    const char* who = "cp_online_multi_adapt_map_sweep";
    const OlMapSweep a{rms, n_windows, mean_std, map_src, map_fill, n_maps, n_classes, expected_slot, chunk_rows, scratch, scratch_bytes,
                       pred, voted, scores, class_hits};
    return olmap_sweep(who, cfg, [&](OlWS* w) { return olam_check_stream(who, cfg, n_streams, max_rows, ws, ws_bytes, index, w); }, true,
                       ws, a, stream);
}

// ---------------------------------------------------------------------------------------
// cue realignment (csrc/online_realign.cuh): a window's activity from the normalised windows, and per cued segment the onset and
// offset of the movement as the activity shows them.  No workspace: everything is the caller's
// ---------------------------------------------------------------------------------------
static_assert(OR_MAXREGION == CP_ONLINE_REALIGN_MAX_REGION && OR_MAXACT == CP_ONLINE_REALIGN_MAX_ACTIVITY && OR_C == CP_EMG_DIM,
              "realign limits");
static_assert(sizeof(OrConfig) == sizeof(cp_online_realign_config), "realign config");

extern "C" int cp_online_realign_activity(const float* windows, int32_t ldw, int64_t n_rows, const float* base, const float* gain,
                                          int32_t* activity, void* stream) {
    const char* who = "cp_online_realign_activity";
    if (n_rows < 1 || n_rows > INT32_MAX) return ol_fail(CP_ERR_ARG, who, "n_rows outside 1..2^31-1");
    if (ldw < CP_EMG_DIM) return ol_fail(CP_ERR_ARG, who, "ldw must be at least 12");
    if (!windows || !base || !gain || !activity) return ol_fail(CP_ERR_ARG, who, "windows, base, gain and activity are required");
    if ((uintptr_t)windows % 4 || (uintptr_t)base % 4 || (uintptr_t)gain % 4 || (uintptr_t)activity % 4)
        return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    OrActivityArgs a{};
    a.windows = windows; a.ldw = ldw; a.n_rows = n_rows; a.activity = activity;
    for (int c = 0; c < OR_C; ++c) {
        a.base[c] = base[c];
        a.gain[c] = gain[c];
    }
    hipLaunchKernelGGL(or_activity_kernel, dim3((unsigned)((n_rows + OR_THREADS - 1) / OR_THREADS)), dim3(OR_THREADS), 0,
                       (hipStream_t)stream, a);
    CKL("or_activity_kernel");
    return 0;
}

extern "C" int cp_online_realign(const int32_t* activity, const int32_t* cue, int64_t n_rows, const int32_t* segments,
                                 int32_t n_segments, const cp_online_realign_config* cfg, int32_t* out_expected,
                                 int32_t* out_segments, int64_t* out_sums, void* stream) {
    const char* who = "cp_online_realign";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_rows < 1 || n_rows > INT32_MAX) return bad("n_rows outside 1..2^31-1");
    if (n_segments < 1 || n_segments > 65536) return bad("n_segments outside 1..65536");
    if (!cfg) return bad("config is required");
    if (cfg->max_lag < 0 || cfg->max_lag > 1024) return bad("max_lag outside 0..1024");
    if (cfg->max_lead < 0 || cfg->max_lead > 1024) return bad("max_lead outside 0..1024");
    if (cfg->context < 0 || cfg->context > 2048) return bad("context outside 0..2048");
    if (cfg->min_len < 1) return bad("min_len must be at least 1");
    if (cfg->min_rest < 1) return bad("min_rest must be at least 1");
    if (cfg->guard < 0 || (int64_t)cfg->min_len <= 2 * (int64_t)cfg->guard) 
        return bad("guard must not be negative, and min_len must exceed 2 guard");
    if (cfg->min_contrast < 0 || cfg->min_contrast > CP_ONLINE_REALIGN_MAX_ACTIVITY) return bad("min_contrast outside 0..4095");
    if (!activity || !cue || !segments || !out_expected || !out_segments || !out_sums)
        return bad("activity, cue, segments, out_expected, out_segments and out_sums are required");
    if ((uintptr_t)activity % 4 || (uintptr_t)cue % 4 || (uintptr_t)segments % 4 || (uintptr_t)out_expected % 4 ||
        (uintptr_t)out_segments % 4 || (uintptr_t)out_sums % 8)
        return bad("misaligned argument");
    OrArgs a{};
    a.activity = activity; a.cue = cue; a.n_rows = (int)n_rows; a.segments = segments; a.n_segments = n_segments;
    a.expected = out_expected; a.out_segments = out_segments; a.out_sums = (long long*)out_sums;
    // a pair is at most the region long and a found one longer than 2 guard: beyond the region's limit the three mean the same
    const int32_t cap = CP_ONLINE_REALIGN_MAX_REGION + 1;
    a.c.max_lag = cfg->max_lag; a.c.max_lead = cfg->max_lead; a.c.context = cfg->context; a.c.min_contrast = cfg->min_contrast;
    a.c.min_len = cfg->min_len < cap ? cfg->min_len : cap;
    a.c.min_rest = cfg->min_rest < cap ? cfg->min_rest : cap;
    a.c.guard = cfg->guard < cap ? cfg->guard : cap;
    hipLaunchKernelGGL(or_default_kernel, dim3((unsigned)((n_rows + OR_THREADS - 1) / OR_THREADS)), dim3(OR_THREADS), 0,
                       (hipStream_t)stream, cue, (long long)n_rows, out_expected);
    CKL("or_default_kernel");
    hipLaunchKernelGGL(or_segment_kernel, dim3(n_segments), dim3(OR_THREADS), 0, (hipStream_t)stream, a);
    CKL("or_segment_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// prototype tracking (csrc/online_track.cuh): one OtState per stream in a workspace of its own, behind any decoder's embeddings
// ---------------------------------------------------------------------------------------
static_assert(OT_MAXK == CP_ONLINE_MAX_CLASSES && OT_MAXVOTE == CP_ONLINE_MAX_VOTE && OT_MAXM == CP_ONLINE_MAX_WINDOWS && OT_D == CP_D_E &&
              OT_SCORES == CP_ONLINE_TRACK_SCORES, "tracker limits");
static_assert(sizeof(OtConfig) == sizeof(cp_online_track_config) && offsetof(OtConfig, rate) == offsetof(cp_online_track_config, rate) &&
              offsetof(OtConfig, min_anchor_cosine) == offsetof(cp_online_track_config, min_anchor_cosine),
              "the sweep reads cp_online_track_config from the device as OtConfig");
static_assert(sizeof(OtState) == 16 + 4 * (OT_MAXK + OT_MAXVOTE) + 16 * OT_MAXK + 8 * OT_MAXK * OT_D + 8 * OT_MAXK * OT_D &&
              offsetof(OtState, anchor) == 2320 && sizeof(OtState) % 16 == 0, "OtState as PrototypeTracker.state reads it back");
static_assert(offsetof(OlState, table) == 3576 && sizeof(OlState) == 7672,
              "PrototypeTracker takes its anchor from the decoders' normalised class table, where their workspace keeps it");

static OtConfig ot_config(const cp_online_track_config* c) {
    OtConfig o{};
    o.vote = c->vote; o.agree = c->agree; o.rate = c->rate;
    o.min_cosine = c->min_cosine; o.min_margin = c->min_margin; o.min_anchor_cosine = c->min_anchor_cosine;
    return o;
}

static int ot_check_config(const char* who, const cp_online_track_config* c) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!c) return bad("config is required");
    if (c->vote < 1 || c->vote > CP_ONLINE_MAX_VOTE) return bad("vote outside 1..256");
    if (!(c->rate >= 0.0 && c->rate < 1.0)) return bad("rate must lie in [0, 1)");
    if (c->agree != 0 && c->agree != 1) return bad("agree must be 0 or 1");
    if (std::isnan(c->min_cosine) || std::isnan(c->min_margin) || std::isnan(c->min_anchor_cosine))
        return bad("min_cosine, min_margin and min_anchor_cosine must not be NaN");
    return 0;
}

static int ot_check(const char* who, const cp_online_track_config* c, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!ws) return bad("config and workspace are required");
    if (int e = ot_check_config(who, c)) return e;
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes < (size_t)n_streams * sizeof(OtState)) return bad("workspace too small");
    return 0;
}

extern "C" size_t cp_online_track_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(OtState));
}

extern "C" int cp_online_track_set_rows(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                        const int32_t* ids, const float* rows, int32_t n_classes, void* stream) {
    const char* who = "cp_online_track_set_rows";
    if (int e = ot_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if (!ids || !rows || n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return ol_fail(CP_ERR_ARG, who, "1..64 classes, with ids and rows");
    if ((uintptr_t)ids % 4 || (uintptr_t)rows % 4) return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    OtIds c{};
    c.K = n_classes;
    for (int k = 0; k < n_classes; ++k) {
        if (ids[k] < 0 || ids[k] == INT32_MAX || (k > 0 && ids[k] <= ids[k - 1]))
            return ol_fail(CP_ERR_ARG, who, "ids must be ascending, distinct and in 0..2^31-2");
        c.ids[k] = ids[k];
    }
    hipLaunchKernelGGL(ot_set_rows_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OtState*)ws + index, c, rows);
    CKL("ot_set_rows_kernel");
    return 0;
}

extern "C" int cp_online_track_reset(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                     int32_t what, void* stream) {
    const char* who = "cp_online_track_reset";
    if (int e = ot_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return ol_fail(CP_ERR_ARG, who, "stream index outside -1..n_streams-1");
    if (what != CP_ONLINE_TRACK_RESET_RING && what != CP_ONLINE_TRACK_RESET_ROWS)
        return ol_fail(CP_ERR_ARG, who, "what must be CP_ONLINE_TRACK_RESET_RING or CP_ONLINE_TRACK_RESET_ROWS");
    hipLaunchKernelGGL(ot_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(64), 0, (hipStream_t)stream, (OtState*)ws,
                       index < 0 ? 0 : index, (int)what);
    CKL("ot_reset_kernel");
    return 0;
}

extern "C" int cp_online_track_push(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes,
                                    const float* embeddings, const int32_t* row0, const int32_t* m, int32_t total_rows, int32_t* pred,
                                    int32_t* voted, float* logits, int32_t ldl, int32_t* updated, void* stream) {
    const char* who = "cp_online_track_push";
    if (int e = ot_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return ol_fail(CP_ERR_ARG, who, "total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (!embeddings || !row0 || !m || !pred || !voted || !updated)
        return ol_fail(CP_ERR_ARG, who, "embeddings, row0, m, pred, voted and updated are required");
    if (logits && (ldl < 1 || ldl > CP_ONLINE_MULTI_MAX_ROWS)) return ol_fail(CP_ERR_ARG, who, "ldl must be at least 1");
    if ((uintptr_t)embeddings % 16) return ol_fail(CP_ERR_ARG, who, "embeddings must be 16-byte aligned");
    if ((uintptr_t)row0 % 4 || (uintptr_t)m % 4 || (uintptr_t)pred % 4 || (uintptr_t)voted % 4 || (uintptr_t)logits % 4 ||
        (uintptr_t)updated % 4)
        return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    OtPushArgs a{};
    a.states = (OtState*)ws; a.emb = embeddings; a.row0 = row0; a.m = m; a.total_rows = total_rows; a.ldl = logits ? ldl : 0;
    a.pred = pred; a.voted = voted; a.logits = logits; a.updated = updated; a.c = ot_config(cfg);
    hipLaunchKernelGGL(ot_push_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    CKL("ot_push_kernel");
    return 0;
}

extern "C" int cp_online_track_rows(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                    float* rows_out, int64_t* n_updates_out, int64_t* n_refused_out, void* stream) {
    const char* who = "cp_online_track_rows";
    if (int e = ot_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if ((uintptr_t)rows_out % 4 || (uintptr_t)n_updates_out % 8 || (uintptr_t)n_refused_out % 8)
        return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    const OtState* st = (const OtState*)ws + index;
    hipStream_t s = (hipStream_t)stream;
    if (rows_out) CK(hipMemcpyAsync(rows_out, st->row, sizeof st->row, hipMemcpyDeviceToDevice, s));
    if (n_updates_out) CK(hipMemcpyAsync(n_updates_out, st->n_updates, sizeof st->n_updates, hipMemcpyDeviceToDevice, s));
    if (n_refused_out) CK(hipMemcpyAsync(n_refused_out, st->n_refused, sizeof st->n_refused, hipMemcpyDeviceToDevice, s));
    return 0;
}

// tracker sweep: n_configs settings over one recording's embeddings, one wave each, from a fresh tracker (ot_sweep_kernel)
extern "C" int cp_online_track_sweep(const float* embeddings, int64_t n_rows, int32_t n_classes, const float* rows,
                                     const int32_t* expected_slot, int64_t tail_from, const cp_online_track_config* configs,
                                     int32_t n_configs, int64_t* scores, int32_t* pred, int32_t* voted, int32_t* updated, void* stream) {
    const char* who = "cp_online_track_sweep";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return bad("n_classes outside 1..64");
    if (n_configs < 1 || n_configs > CP_ONLINE_TRACK_SWEEP_MAX_CONFIGS) return bad("n_configs outside 1..65536");
    if (n_rows < 1 || n_rows > INT32_MAX) return bad("n_rows outside 1..2^31-1");
    if (tail_from < 0) return bad("tail_from must not be negative");
    if (!embeddings || !rows || !expected_slot || !configs || !scores)
        return bad("embeddings, rows, expected_slot, configs and scores are required");
    if ((uintptr_t)embeddings % 16) return bad("embeddings must be 16-byte aligned");
    if ((uintptr_t)rows % 4 || (uintptr_t)expected_slot % 4 || (uintptr_t)configs % 8 || (uintptr_t)scores % 8 || (uintptr_t)pred % 4 ||
        (uintptr_t)voted % 4 || (uintptr_t)updated % 4)
        return bad("misaligned argument");
    OtSweepArgs a{};
    a.emb = embeddings; a.expected = expected_slot; a.configs = (const OtConfig*)configs; a.rows = rows; a.n_rows = n_rows;
    a.tail_from = tail_from; a.n_configs = n_configs; a.K = n_classes; a.scores = (long long*)scores; a.pred = pred; a.voted = voted;
    a.updated = updated;
    hipLaunchKernelGGL(ot_sweep_kernel, dim3((n_configs + OT_SWEEP_WAVES - 1) / OT_SWEEP_WAVES), dim3(64 * OT_SWEEP_WAVES), 0,
                       (hipStream_t)stream, a);
    CKL("ot_sweep_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// held-out enrolment scoring (csrc/online_holdout.cuh): sums per training mask, rows per plan, one wave per plan over the
// evaluated windows, and the held-out logits.  Plans and masks live on the device and are checked by the kernels.
// ---------------------------------------------------------------------------------------
static_assert(OH_SCORES == CP_ONLINE_HOLDOUT_SCORES && OH_MAX_PLANS == CP_ONLINE_HOLDOUT_MAX_PLANS &&
              OH_MAX_REPS == CP_ONLINE_HOLDOUT_MAX_REPS && OH_MAXK == CP_ONLINE_MAX_CLASSES && OH_D == CP_D_E, "hold-out constants");
static_assert(sizeof(OhPlan) == sizeof(cp_online_holdout_plan) && sizeof(OhPlan) == 24 &&
              offsetof(OhPlan, sums_index) == offsetof(cp_online_holdout_plan, sums_index) &&
              offsetof(OhPlan, mix) == offsetof(cp_online_holdout_plan, mix), "the kernels read cp_online_holdout_plan as OhPlan");
static_assert(sizeof(OlState) == 7672 && sizeof(OlmMeta) == 16 && sizeof(OlaHead) == 16 && OLAM_STATS * 8 == 9 * 2 * 512 * 8,
              "holdout.score_enrolment keeps a copy of what ol_carve lays in front of the weights and puts it back");

// what the four entries share: the recording's size and class count
static int oh_check_shape(const char* who, int64_t n_rows, int32_t n_classes) {
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return ol_fail(CP_ERR_ARG, who, "n_classes outside 1..64");
    if (n_rows < 1 || n_rows > INT32_MAX) return ol_fail(CP_ERR_ARG, who, "n_rows outside 1..2^31-1");
    return 0;
}

extern "C" int cp_online_holdout_sums(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot,
                                      const int32_t* rep, const uint32_t* train_masks, int32_t n_masks, double* sums, void* stream) {
    const char* who = "cp_online_holdout_sums";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (int e = oh_check_shape(who, n_rows, n_classes)) return e;
    if (n_masks < 1 || n_masks > CP_ONLINE_HOLDOUT_MAX_PLANS) return bad("n_masks outside 1..4096");
    if (!embeddings || !slot || !rep || !train_masks || !sums) return bad("embeddings, slot, rep, train_masks and sums are required");
    if ((uintptr_t)embeddings % 16) return bad("embeddings must be 16-byte aligned");
    if ((uintptr_t)slot % 4 || (uintptr_t)rep % 4 || (uintptr_t)train_masks % 4 || (uintptr_t)sums % 8) return bad("misaligned argument");
    hipLaunchKernelGGL(oh_sums_kernel, dim3((n_masks + OH_SUM_MASKS - 1) / OH_SUM_MASKS, OH_MAXK), dim3(64), 0, (hipStream_t)stream,
                       embeddings, (long long)n_rows, (int)n_classes, slot, rep, train_masks, (int)n_masks, sums);
    CKL("oh_sums_kernel");
    return 0;
}

extern "C" int cp_online_holdout_tables(const double* sums, int32_t n_masks, int32_t n_classes, const float* prior,
                                        const cp_online_holdout_plan* plans, int32_t n_plans, float* rows, float* unit, void* stream) {
    const char* who = "cp_online_holdout_tables";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return bad("n_classes outside 1..64");
    if (n_masks < 1 || n_masks > CP_ONLINE_HOLDOUT_MAX_PLANS) return bad("n_masks outside 1..4096");
    if (n_plans < 1 || n_plans > CP_ONLINE_HOLDOUT_MAX_PLANS) return bad("n_plans outside 1..4096");
    if (!sums || !prior || !plans || !rows || !unit) return bad("sums, prior, plans, rows and unit are required");
    if ((uintptr_t)sums % 8 || (uintptr_t)plans % 8 || (uintptr_t)prior % 4 || (uintptr_t)rows % 4 || (uintptr_t)unit % 16)
        return bad("misaligned argument (unit: 16 bytes)");
    hipLaunchKernelGGL(oh_tables_kernel, dim3(n_plans), dim3(64), 0, (hipStream_t)stream, sums, (int)n_masks, (int)n_classes, prior,
                       (const OhPlan*)plans, rows, unit);
    CKL("oh_tables_kernel");
    return 0;
}

extern "C" int cp_online_holdout_score(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot,
                                       const int32_t* rep, const float* unit, const cp_online_holdout_plan* plans, int32_t n_plans,
                                       int32_t vote, int64_t* scores, int32_t* confusion, int32_t* voted_confusion, int32_t* pred,
                                       int32_t* voted, void* stream) {
    const char* who = "cp_online_holdout_score";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (int e = oh_check_shape(who, n_rows, n_classes)) return e;
    if (n_plans < 1 || n_plans > CP_ONLINE_HOLDOUT_MAX_PLANS) return bad("n_plans outside 1..4096");
    if (vote < 1 || vote > CP_ONLINE_MAX_VOTE) return bad("vote outside 1..256");
    if (!embeddings || !slot || !rep || !unit || !plans || !scores) return bad("embeddings, slot, rep, unit, plans and scores are required");
    if ((uintptr_t)embeddings % 16 || (uintptr_t)unit % 16) return bad("embeddings and unit must be 16-byte aligned");
    if ((uintptr_t)slot % 4 || (uintptr_t)rep % 4 || (uintptr_t)plans % 8 || (uintptr_t)scores % 8 || (uintptr_t)confusion % 4 ||
        (uintptr_t)voted_confusion % 4 || (uintptr_t)pred % 4 || (uintptr_t)voted % 4)
        return bad("misaligned argument");
    OhScoreArgs a{};
    a.emb = embeddings; a.slot = slot; a.rep = rep; a.unit = unit; a.plans = (const OhPlan*)plans; a.n_rows = n_rows;
    a.n_plans = n_plans; a.K = n_classes; a.vote = vote; a.scores = (long long*)scores; a.confusion = confusion;
    a.voted_confusion = voted_confusion; a.pred = pred; a.voted = voted;
    if (confusion || voted_confusion) {
        hipLaunchKernelGGL(oh_score_kernel<true>, dim3(n_plans), dim3(64), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(oh_score_kernel<false>, dim3(n_plans), dim3(64), 0, (hipStream_t)stream, a);
    }
    CKL("oh_score_kernel");
    return 0;
}

extern "C" int cp_online_holdout_logits(const float* embeddings, int64_t n_rows, int32_t n_classes, const float* unit, int32_t n_plans,
                                        const int32_t* assign, float* logits, int32_t ldl, void* stream) {
    const char* who = "cp_online_holdout_logits";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (int e = oh_check_shape(who, n_rows, n_classes)) return e;
    if (n_plans < 1 || n_plans > CP_ONLINE_HOLDOUT_MAX_PLANS) return bad("n_plans outside 1..4096");
    if (ldl < n_classes) return bad("ldl must be at least n_classes");
    if (!embeddings || !unit || !assign || !logits) return bad("embeddings, unit, assign and logits are required");
    if ((uintptr_t)embeddings % 4 || (uintptr_t)unit % 4 || (uintptr_t)assign % 4 || (uintptr_t)logits % 4) return bad("misaligned argument");
    hipLaunchKernelGGL(oh_logits_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, embeddings,
                       (long long)n_rows, (int)n_classes, unit, (int)n_plans, assign, logits, (int)ldl);
    CKL("oh_logits_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// posture prototypes (csrc/online_prototypes.cuh): the fit of up to four rows per class in one launch, and the group stage
// behind any decoder's logits, one OpgState per stream in a workspace of its own
// ---------------------------------------------------------------------------------------
static_assert(OP_MAXR == CP_ONLINE_PROTO_MAX_ROWS && OP_MAX_ITERS == CP_ONLINE_PROTO_MAX_ITERS && OP_MAXK == CP_ONLINE_MAX_CLASSES &&
              OP_D == CP_D_E && OPG_MAXM == CP_ONLINE_MAX_WINDOWS && OP_MAXR * OP_D == 64, "posture prototype constants");
static_assert(sizeof(OpgState) == 4 * (4 + 3 * OP_MAXK + OL_MAXVOTE), "OpgState is 452 words");

extern "C" int cp_online_proto_fit(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot, const uint8_t* use,
                                   const int32_t* rows_per_class, int32_t iters, int32_t min_windows, float* rows, int64_t* counts,
                                   uint8_t* valid, int64_t* moved, int32_t* assign, void* stream) {
    const char* who = "cp_online_proto_fit";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (int e = oh_check_shape(who, n_rows, n_classes)) return e;
    if (iters < 0 || iters > CP_ONLINE_PROTO_MAX_ITERS) return bad("iters outside 0..64");
    if (min_windows < 1) return bad("min_windows must be at least 1");
    if (!embeddings || !slot || !rows_per_class || !rows || !counts || !valid || !assign || (iters > 0 && !moved))
        return bad("embeddings, slot, rows_per_class, rows, counts, valid, assign (and moved, with iters > 0) are required");
    if ((uintptr_t)embeddings % 16) return bad("embeddings must be 16-byte aligned");
    if ((uintptr_t)slot % 4 || (uintptr_t)rows_per_class % 4 || (uintptr_t)rows % 4 || (uintptr_t)counts % 8 || (uintptr_t)moved % 8 ||
        (uintptr_t)assign % 4)
        return bad("misaligned argument");
    OpFitArgs a{};
    int total = 0;
    for (int c = 0; c < n_classes; ++c) {
        if (rows_per_class[c] < 1 || rows_per_class[c] > CP_ONLINE_PROTO_MAX_ROWS) return bad("rows_per_class outside 1..4");
        a.rows_per_class[c] = (unsigned char)rows_per_class[c];
        total += rows_per_class[c];
    }
    if (total > CP_ONLINE_MAX_CLASSES) return bad("rows_per_class sums to more than 64 rows");
    a.emb = embeddings; a.slot = slot; a.use = use; a.n_rows = n_rows; a.K = n_classes; a.iters = iters; a.min_windows = min_windows;
    a.rows = rows; a.counts = (long long*)counts; a.valid = valid; a.moved = (long long*)moved; a.assign = assign;
    hipLaunchKernelGGL(op_fit_kernel, dim3(n_classes + 1), dim3(64), 0, (hipStream_t)stream, a);
    CKL("op_fit_kernel");
    return 0;
}

static int opg_check(const char* who, int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!ws) return bad("workspace is required");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if (vote < 1 || vote > CP_ONLINE_MAX_VOTE) return bad("vote outside 1..256");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes < (size_t)n_streams * sizeof(OpgState)) return bad("workspace too small");
    return 0;
}

extern "C" size_t cp_online_group_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(OpgState));
}

extern "C" int cp_online_group_set_groups(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                          const int32_t* row_ids, const int32_t* class_of_row, int32_t n_rows, void* stream) {
    const char* who = "cp_online_group_set_groups";
    if (int e = opg_check(who, vote, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if (!row_ids || !class_of_row || n_rows < 1 || n_rows > CP_ONLINE_MAX_CLASSES)
        return ol_fail(CP_ERR_ARG, who, "1..64 rows, with row_ids and class_of_row");
    OpgGroups g{};
    g.R = n_rows;
    for (int r = 0; r < n_rows; ++r) {
        if (row_ids[r] < 0 || row_ids[r] == INT32_MAX || (r > 0 && row_ids[r] <= row_ids[r - 1]))
            return ol_fail(CP_ERR_ARG, who, "row_ids must be ascending, distinct and in 0..2^31-2");
        if (class_of_row[r] < 0 || class_of_row[r] == INT32_MAX) return ol_fail(CP_ERR_ARG, who, "class ids must lie in 0..2^31-2");
        g.row_ids[r] = row_ids[r];
        int at = 0;                                            // group ids stay ascending: insert a new class id in its place
        while (at < g.G && g.group_ids[at] < class_of_row[r]) ++at;
        if (at == g.G || g.group_ids[at] != class_of_row[r]) {
            for (int i = g.G; i > at; --i) g.group_ids[i] = g.group_ids[i - 1];
            g.group_ids[at] = class_of_row[r];
            ++g.G;
        }
    }
    for (int r = 0; r < n_rows; ++r) {
        int at = 0;
        while (g.group_ids[at] != class_of_row[r]) ++at;
        g.group_of[r] = at;
    }
    hipLaunchKernelGGL(opg_set_groups_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OpgState*)ws + index, g);
    CKL("opg_set_groups_kernel");
    return 0;
}

extern "C" int cp_online_group_reset(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream) {
    const char* who = "cp_online_group_reset";
    if (int e = opg_check(who, vote, n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return ol_fail(CP_ERR_ARG, who, "stream index outside -1..n_streams-1");
    hipLaunchKernelGGL(opg_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(64), 0, (hipStream_t)stream, (OpgState*)ws,
                       index < 0 ? 0 : index);
    CKL("opg_reset_kernel");
    return 0;
}

extern "C" int cp_online_group_push(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, const float* logits, int32_t ldl,
                                    const int32_t* row0, const int32_t* m, int32_t total_rows, int32_t* pred, int32_t* voted,
                                    int32_t* row, float* class_logits, int32_t ldc, void* stream) {
    const char* who = "cp_online_group_push";
    if (int e = opg_check(who, vote, n_streams, ws, ws_bytes)) return e;
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return ol_fail(CP_ERR_ARG, who, "total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (ldl < 1) return ol_fail(CP_ERR_ARG, who, "ldl must be at least 1");
    if (class_logits && ldc < 1) return ol_fail(CP_ERR_ARG, who, "ldc must be at least 1");
    if (!logits || !row0 || !m || !pred || !voted || !row) return ol_fail(CP_ERR_ARG, who, "logits, row0, m, pred, voted and row are required");
    if ((uintptr_t)logits % 4 || (uintptr_t)row0 % 4 || (uintptr_t)m % 4 || (uintptr_t)pred % 4 || (uintptr_t)voted % 4 ||
        (uintptr_t)row % 4 || (uintptr_t)class_logits % 4)
        return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    OpgPushArgs a{};
    a.states = (OpgState*)ws; a.logits = logits; a.row0 = row0; a.m = m; a.ldl = ldl; a.total_rows = total_rows; a.vote = vote;
    a.ldc = class_logits ? ldc : 0; a.pred = pred; a.voted = voted; a.row = row; a.class_logits = class_logits;
    hipLaunchKernelGGL(opg_push_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    CKL("opg_push_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// user metric (csrc/online_metric.cuh): the moments of a cued recording, the shrunk and factored within-class scatter, the
// transform of a recording, and the stage behind any decoder's embeddings, one OmState per stream in a workspace of its own
// ---------------------------------------------------------------------------------------
static_assert(OM_MAXK == CP_ONLINE_MAX_CLASSES && OM_D == CP_D_E && OM_MAXM == CP_ONLINE_MAX_WINDOWS && OM_MOMENTS == CP_ONLINE_METRIC_MOMENTS &&
              OM_MAX_SHRINKS == CP_ONLINE_METRIC_MAX_SHRINKS && OM_APPLY_THREADS == OM_D * OM_D, "user metric constants");
static_assert(sizeof(OmState) == 4 * (4 + OM_MAXK + OL_MAXVOTE + OM_D * OM_D + OM_MAXK * OM_D) && offsetof(OmState, A) == 4 * (4 + OM_MAXK + OL_MAXVOTE) &&
              sizeof(OmState) % 16 == 0 && offsetof(OmState, row) % 16 == 0, "OmState as MetricRows.state reads it back");

extern "C" int cp_online_metric_moments(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot, const uint8_t* use,
                                        double* moments, int64_t* counts, void* stream) {
    const char* who = "cp_online_metric_moments";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (int e = oh_check_shape(who, n_rows, n_classes)) return e;
    if (!embeddings || !slot || !moments || !counts) return bad("embeddings, slot, moments and counts are required");
    if ((uintptr_t)embeddings % 16) return bad("embeddings must be 16-byte aligned");
    if ((uintptr_t)slot % 4 || (uintptr_t)moments % 8 || (uintptr_t)counts % 8) return bad("misaligned argument");
    hipLaunchKernelGGL(om_moments_kernel, dim3(n_classes), dim3(64), 0, (hipStream_t)stream, embeddings, (long long)n_rows, slot, use,
                       moments, (long long*)counts);
    CKL("om_moments_kernel");
    return 0;
}

extern "C" int cp_online_metric_factor(const double* moments, const int64_t* counts, int32_t n_classes, int32_t min_windows,
                                       const double* shrinks, int32_t n_shrinks, float* A, uint8_t* valid, void* stream) {
    const char* who = "cp_online_metric_factor";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return bad("n_classes outside 1..64");
    if (min_windows < 1) return bad("min_windows must be at least 1");
    if (n_shrinks < 1 || n_shrinks > CP_ONLINE_METRIC_MAX_SHRINKS) return bad("n_shrinks outside 1..64");
    if (!moments || !counts || !shrinks || !A || !valid) return bad("moments, counts, shrinks, A and valid are required");
    if ((uintptr_t)moments % 8 || (uintptr_t)counts % 8 || (uintptr_t)shrinks % 8 || (uintptr_t)A % 4) return bad("misaligned argument");
    OmFactorArgs a{};
    for (int t = 0; t < n_shrinks; ++t) {
        if (!(shrinks[t] >= 0.0 && shrinks[t] <= 1.0)) return bad("every shrink value must lie in [0, 1]");
        a.shrinks[t] = shrinks[t];
    }
    a.moments = moments; a.counts = (const long long*)counts; a.K = n_classes; a.min_windows = min_windows; a.n_shrinks = n_shrinks;
    a.A = A; a.valid = valid;
    hipLaunchKernelGGL(om_factor_kernel, dim3(n_shrinks), dim3(64), 0, (hipStream_t)stream, a);
    CKL("om_factor_kernel");
    return 0;
}

extern "C" int cp_online_metric_apply(const float* embeddings, int64_t n_rows, const float* A, float* out, void* stream) {
    const char* who = "cp_online_metric_apply";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_rows < 1 || n_rows > INT32_MAX) return bad("n_rows outside 1..2^31-1");
    if (!embeddings || !A || !out) return bad("embeddings, A and out are required");
    if ((uintptr_t)embeddings % 16 || (uintptr_t)out % 16) return bad("embeddings and out must be 16-byte aligned");
    if ((uintptr_t)A % 4) return bad("misaligned argument");
    hipLaunchKernelGGL(om_apply_kernel, dim3((unsigned)((n_rows + OM_APPLY_THREADS - 1) / OM_APPLY_THREADS)), dim3(OM_APPLY_THREADS), 0,
                       (hipStream_t)stream, embeddings, (long long)n_rows, A, out);
    CKL("om_apply_kernel");
    return 0;
}

extern "C" size_t cp_online_metric_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(OmState));
}

static int om_check(const char* who, int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!ws) return bad("workspace is required");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if (vote < 1 || vote > CP_ONLINE_MAX_VOTE) return bad("vote outside 1..256");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes != cp_online_metric_workspace_bytes(n_streams)) return bad("ws_bytes is not cp_online_metric_workspace_bytes(n_streams)");
    return 0;
}

extern "C" int cp_online_metric_set(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, const float* A,
                                    const float* rows, const int32_t* ids, int32_t n_classes, void* stream) {
    const char* who = "cp_online_metric_set";
    if (int e = om_check(who, vote, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if (!A && !rows) return ol_fail(CP_ERR_ARG, who, "A or rows is required");
    if ((uintptr_t)A % 4 || (uintptr_t)rows % 4 || (uintptr_t)ids % 4) return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    OmIds c{};
    if (rows) {
        if (!ids || n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return ol_fail(CP_ERR_ARG, who, "rows come with 1..64 classes and their ids");
        c.K = n_classes;
        for (int k = 0; k < n_classes; ++k) {
            if (ids[k] < 0 || ids[k] == INT32_MAX || (k > 0 && ids[k] <= ids[k - 1]))
                return ol_fail(CP_ERR_ARG, who, "ids must be ascending, distinct and in 0..2^31-2");
            c.ids[k] = ids[k];
        }
    }
    hipLaunchKernelGGL(om_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OmState*)ws + index, A, rows, c);
    CKL("om_set_kernel");
    return 0;
}

extern "C" int cp_online_metric_reset(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, int32_t what,
                                      void* stream) {
    const char* who = "cp_online_metric_reset";
    if (int e = om_check(who, vote, n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return ol_fail(CP_ERR_ARG, who, "stream index outside -1..n_streams-1");
    if (what != CP_ONLINE_METRIC_RESET_RING && what != CP_ONLINE_METRIC_RESET_ALL)
        return ol_fail(CP_ERR_ARG, who, "what must be CP_ONLINE_METRIC_RESET_RING or CP_ONLINE_METRIC_RESET_ALL");
    hipLaunchKernelGGL(om_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(64), 0, (hipStream_t)stream, (OmState*)ws,
                       index < 0 ? 0 : index, (int)what);
    CKL("om_reset_kernel");
    return 0;
}

extern "C" int cp_online_metric_push(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, const float* embeddings,
                                     const int32_t* row0, const int32_t* m, int32_t total_rows, int32_t* pred, int32_t* voted,
                                     float* logits, int32_t ldl, void* stream) {
    const char* who = "cp_online_metric_push";
    if (int e = om_check(who, vote, n_streams, ws, ws_bytes)) return e;
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return ol_fail(CP_ERR_ARG, who, "total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (!embeddings || !row0 || !m || !pred || !voted) return ol_fail(CP_ERR_ARG, who, "embeddings, row0, m, pred and voted are required");
    if (logits && (ldl < 1 || ldl > CP_ONLINE_MULTI_MAX_ROWS)) return ol_fail(CP_ERR_ARG, who, "ldl must be at least 1");
    if ((uintptr_t)embeddings % 16) return ol_fail(CP_ERR_ARG, who, "embeddings must be 16-byte aligned");
    if ((uintptr_t)row0 % 4 || (uintptr_t)m % 4 || (uintptr_t)pred % 4 || (uintptr_t)voted % 4 || (uintptr_t)logits % 4)
        return ol_fail(CP_ERR_ARG, who, "misaligned argument");
    OmPushArgs a{};
    a.states = (OmState*)ws; a.emb = embeddings; a.row0 = row0; a.m = m; a.total_rows = total_rows; a.ldl = logits ? ldl : 0;
    a.vote = vote; a.pred = pred; a.voted = voted; a.logits = logits;
    hipLaunchKernelGGL(om_push_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    CKL("om_push_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------
// closed-form head fit (csrc/online_readout.cuh): the weighted moments of a recording's tail inputs per group, the ridge
// normal equations of many plans solved by Cholesky, and the fitted projections applied as the push's tail applies its own
// ---------------------------------------------------------------------------------------
static_assert(OLR_MAXK == CP_ONLINE_MAX_CLASSES && OLR_MAX_GROUPS == CP_ONLINE_READOUT_MAX_GROUPS && OLR_MAX_PLANS == CP_ONLINE_READOUT_MAX_PLANS &&
              OLR_STAGE == CP_ONLINE_READOUT_STAGE && OLR_X == CP_ONLINE_READOUT_X, "readout constants");
static_assert(sizeof(OlrSolveArgs) <= 4096, "olr_solve_kernel takes its plans as kernel arguments");

// One scratch serves the three entries in turn: the index lists and their lengths (moments), a matrix per plan
// (solve), the fitted projections in the compute dtype, sized for f32 (apply).
static size_t olr_moments_bytes(int64_t n_rows, int32_t n_groups) {
    return align256((size_t)n_groups * (size_t)n_rows * 4) + align256((size_t)OLR_MAX_GROUPS * 4);
}
static size_t olr_solve_bytes(int32_t n_plans) { return align256((size_t)n_plans * OLR_PLAN_DOUBLES * 8); }
static size_t olr_apply_bytes(int32_t n_plans) { return align256((size_t)n_plans * OLF_W * 4); }

extern "C" size_t cp_online_readout_scratch_bytes(int64_t n_rows, int32_t n_groups, int32_t n_plans) {
    if (n_rows < 1) n_rows = 1;
    if (n_groups < 1) n_groups = 1;
    if (n_plans < 1) n_plans = 1;
    size_t n = olr_moments_bytes(n_rows, n_groups);
    if (olr_solve_bytes(n_plans) > n) n = olr_solve_bytes(n_plans);
    if (olr_apply_bytes(n_plans) > n) n = olr_apply_bytes(n_plans);
    return n;
}

extern "C" int cp_online_readout_moments(const void* u, int32_t dtype, int64_t n_rows, const int32_t* slot, const int32_t* group,
                                         const double* weight, const float* targets, int32_t n_classes, int32_t n_groups, double* G,
                                         double* C, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_readout_moments";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (dtype != CP_F32 && dtype != CP_BF16) return bad("dtype must be CP_F32 or CP_BF16");
    if (n_rows < 0 || n_rows > (int64_t)1 << 24) return bad("n_rows outside 0..2**24");
    if (n_classes < 1 || n_classes > CP_ONLINE_MAX_CLASSES) return bad("n_classes outside 1..64");
    if (n_groups < 1 || n_groups > CP_ONLINE_READOUT_MAX_GROUPS) return bad("n_groups outside 1..16");
    if (!targets || !G || !C || !scratch) return bad("targets, G, C and scratch are required");
    if (n_rows > 0 && (!u || !slot || !group || !weight)) return bad("u, slot, group and weight are required");
    if ((uintptr_t)u % 16 || (uintptr_t)slot % 4 || (uintptr_t)group % 4 || (uintptr_t)weight % 8 || (uintptr_t)targets % 4 ||
        (uintptr_t)G % 8 || (uintptr_t)C % 8 || (uintptr_t)scratch % 256)
        return bad("misaligned argument");
    if (scratch_bytes < olr_moments_bytes(n_rows < 1 ? 1 : n_rows, n_groups)) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    int32_t* idx = (int32_t*)scratch;
    int32_t* count = (int32_t*)((unsigned char*)scratch + align256((size_t)n_groups * (size_t)(n_rows < 1 ? 1 : n_rows) * 4));
    hipLaunchKernelGGL(olr_index_kernel, dim3(n_groups), dim3(64), 0, (hipStream_t)stream, slot, group, (int)n_rows, (int)n_classes, idx, count);
    CKL("olr_index_kernel");
    return ol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        OlrMomentsArgs<T> a{};
        a.u = (const T*)u; a.slot = slot; a.weight = weight; a.targets = targets; a.idx = idx; a.count = count; a.G = G; a.C = C;
        a.n_rows = (int)n_rows; a.K = n_classes;
        hipLaunchKernelGGL((olr_moments_kernel<T>), dim3(OLR_TILES, n_groups), dim3(OLR_MOM_THREADS), 0, (hipStream_t)stream, a);
        CKL("olr_moments_kernel");
        return 0;
    });
}

extern "C" int cp_online_readout_solve(const double* G, const double* C, int32_t n_groups, const uint32_t* masks, const double* ridges,
                                       int32_t n_plans, float* W, float* b, int32_t* status, void* scratch, size_t scratch_bytes,
                                       void* stream) {
    const char* who = "cp_online_readout_solve";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_groups < 1 || n_groups > CP_ONLINE_READOUT_MAX_GROUPS) return bad("n_groups outside 1..16");
    if (n_plans < 0 || n_plans > CP_ONLINE_READOUT_MAX_PLANS) return bad("n_plans outside 0..256");
    if (n_plans == 0) return 0;
    if (!G || !C || !masks || !ridges || !W || !b || !status || !scratch) return bad("G, C, masks, ridges, W, b, status and scratch are required");
    if ((uintptr_t)G % 8 || (uintptr_t)C % 8 || (uintptr_t)W % 4 || (uintptr_t)b % 4 || (uintptr_t)status % 4 || (uintptr_t)scratch % 256)
        return bad("misaligned argument");
    OlrSolveArgs a{};
    for (int t = 0; t < n_plans; ++t) {
        if (masks[t] >> n_groups) return bad("a plan's mask names a group at or above n_groups");
        if (!(ridges[t] >= 0.0) || !std::isfinite(ridges[t])) return bad("every ridge must be finite and >= 0");
        a.mask[t] = (unsigned short)masks[t];
        a.ridge[t] = ridges[t];
    }
    if (scratch_bytes < olr_solve_bytes(n_plans)) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    a.G = G; a.C = C; a.scratch = (double*)scratch; a.W = W; a.b = b; a.status = status; a.n_groups = n_groups;
    static bool attr_set = false;
    if (!attr_set) {      // > 64 KiB of dynamic LDS needs the opt-in once per process
        CK(hipFuncSetAttribute((const void*)olr_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, OLR_SOLVE_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL(olr_solve_kernel, dim3(n_plans), dim3(OLR_SOLVE_THREADS), OLR_SOLVE_LDS, (hipStream_t)stream, a);
    CKL("olr_solve_kernel");
    return 0;
}

extern "C" int cp_online_readout_apply(const void* u, int32_t dtype, int64_t n_rows, const float* W, const float* b, int32_t n_plans,
                                       float* out, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_readout_apply";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (dtype != CP_F32 && dtype != CP_BF16) return bad("dtype must be CP_F32 or CP_BF16");
    if (n_rows < 0 || n_rows > (int64_t)1 << 24) return bad("n_rows outside 0..2**24");
    if (n_plans < 0 || n_plans > CP_ONLINE_READOUT_MAX_PLANS) return bad("n_plans outside 0..256");
    if (n_rows == 0 || n_plans == 0) return 0;
    if (!u || !W || !b || !out || !scratch) return bad("u, W, b, out and scratch are required");
    if ((uintptr_t)u % 16 || (uintptr_t)W % 4 || (uintptr_t)b % 4 || (uintptr_t)out % 4 || (uintptr_t)scratch % 256) return bad("misaligned argument");
    if (scratch_bytes < olr_apply_bytes(n_plans)) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    OlrApplyArgs a{};
    a.u = u; a.wT = scratch; a.b = b; a.out = out; a.n_rows = (int)n_rows;
    const long long n = (long long)n_plans * OLF_W;
    return ol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((olr_round_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, (T*)scratch, n);
        CKL("olr_round_kernel");
        hipLaunchKernelGGL((olr_apply_kernel<T>), dim3((unsigned)((n_rows + OLR_APPLY_ROWS - 1) / OLR_APPLY_ROWS), n_plans), dim3(OL_THREADS), 0,
                           (hipStream_t)stream, a);
        CKL("olr_apply_kernel");
        return 0;
    });
}

// ---------------------------------------------------------------------------------------
// per-stream projections of the multi-stream decoders (csrc/online_projections.cuh): a bank of one slot per stream in a buffer
// of the caller's, next to the workspace; the *_proj entries are the push, enrolment and map-sweep entries of the two
// multi-stream forms with that bank.  bank == NULL: the entry they are named after, launch for launch
// ---------------------------------------------------------------------------------------
static size_t olp_bank_bytes(int32_t n_streams, int32_t dtype) {
    return (size_t)n_streams * (dtype == CP_BF16 ? olp_slot_bytes<bf16_t>() : olp_slot_bytes<float>());
}

extern "C" size_t cp_online_projections_bytes(int32_t n_streams, int32_t dtype) {
    if (n_streams < 1) n_streams = 1;
    return olp_bank_bytes(n_streams, dtype);
}

// a bank an entry was given (bank != NULL) for n_streams streams in dtype
static int olp_check_bank(const char* who, int32_t dtype, const void* bank, size_t bank_bytes, int32_t n_streams) {
    if (dtype != CP_F32 && dtype != CP_BF16) return ol_fail(CP_ERR_ARG, who, "dtype must be CP_F32 or CP_BF16 (no 8-bit path)");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return ol_fail(CP_ERR_ARG, who, "n_streams outside 1..256");
    if ((uintptr_t)bank % 256) return ol_fail(CP_ERR_ARG, who, "bank not 256-byte aligned");
    if (bank_bytes < olp_bank_bytes(n_streams, dtype)) return ol_fail(CP_ERR_WORKSPACE, who, "bank too small");
    return 0;
}

// the entries that work on the bank alone; out: slot `index` (index -1, clear only: slot 0)
static int olp_check_slot(const char* who, int32_t dtype, void* bank, size_t bank_bytes, int32_t n_streams, int32_t index, bool all_ok,
                          unsigned char** out) {
    if (!bank) return ol_fail(CP_ERR_ARG, who, "bank is required");
    if (int e = olp_check_bank(who, dtype, bank, bank_bytes, n_streams)) return e;
    if (all_ok ? (index < -1 || index >= n_streams) : (index < 0 || index >= n_streams))
        return ol_fail(CP_ERR_ARG, who, all_ok ? "stream index outside -1..n_streams-1" : "stream index outside 0..n_streams-1");
    *out = (unsigned char*)bank + (size_t)(index < 0 ? 0 : index) * olp_bank_bytes(1, dtype);
    return 0;
}

extern "C" int cp_online_projections_set(int32_t dtype, void* bank, size_t bank_bytes, int32_t n_streams, int32_t index, const float* W,
                                         const float* b, void* stream) {
    const char* who = "cp_online_projections_set";
    unsigned char* slot;
    if (int e = olp_check_slot(who, dtype, bank, bank_bytes, n_streams, index, false, &slot)) return e;
    if (!W || !b) return ol_fail(CP_ERR_ARG, who, "W and b are required");
    if ((uintptr_t)W % 4 || (uintptr_t)b % 4) return ol_fail(CP_ERR_ARG, who, "misaligned W or b");
    return ol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        const OlpSlot sl = olp_slot0(t, slot);
        hipLaunchKernelGGL((olp_set_kernel<T>), dim3(OLF_W / 256), dim3(256), 0, (hipStream_t)stream, W, b, (T*)sl.w, (float*)sl.bias,
                           (unsigned*)sl.set);
        CKL("olp_set_kernel");
        return 0;
    });
}

extern "C" int cp_online_projections_get(int32_t dtype, const void* bank, size_t bank_bytes, int32_t n_streams, int32_t index, float* W,
                                         float* b, int32_t* is_set, void* stream) {
    const char* who = "cp_online_projections_get";
    unsigned char* slot;
    if (int e = olp_check_slot(who, dtype, (void*)bank, bank_bytes, n_streams, index, false, &slot)) return e;
    if (!W || !b) return ol_fail(CP_ERR_ARG, who, "W and b are required");
    if ((uintptr_t)W % 4 || (uintptr_t)b % 4 || (uintptr_t)is_set % 4) return ol_fail(CP_ERR_ARG, who, "misaligned W, b or is_set");
    return ol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((olp_get_kernel<T>), dim3(OLF_W / 256), dim3(256), 0, (hipStream_t)stream, olp_slot0(t, slot), W, b, is_set);
        CKL("olp_get_kernel");
        return 0;
    });
}

extern "C" int cp_online_projections_clear(int32_t dtype, void* bank, size_t bank_bytes, int32_t n_streams, int32_t index, void* stream) {
    const char* who = "cp_online_projections_clear";
    unsigned char* slot;
    if (int e = olp_check_slot(who, dtype, bank, bank_bytes, n_streams, index, true, &slot)) return e;
    return ol_dispatch(dtype, [&](auto t) {
        hipLaunchKernelGGL(olp_clear_kernel, dim3(index < 0 ? n_streams : 1), dim3(64), 0, (hipStream_t)stream,
                           (unsigned char*)olp_slot0(t, slot).set, olp_bank_bytes(1, dtype));
        CKL("olp_clear_kernel");
        return 0;
    });
}

// the two pushes: cp_online_multi*_push_embed and a bank
static int olp_push(const char* who, bool adaptive, const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                    size_t ws_bytes, const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                    const float* mean_std, const OlMap& map, int32_t* pred, int32_t* voted, float* logits, float* windows,
                    size_t bank_bytes, void* stream) {
    if (map.bank) {
        OlWS w;                                               // (the configuration first: the bank is sized by its dtype)
        if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, adaptive, &w)) return e;
        if (int e = olp_check_bank(who, cfg->dtype, map.bank, bank_bytes, n_streams)) return e;
    }
    return olm_push(who, adaptive, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples, total_windows, mean_std, pred, voted,
                    logits, windows, map, stream);
}

extern "C" int cp_online_multi_push_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                         const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                         const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                         int32_t* voted, float* logits, float* windows, float* embeddings, const void* bank,
                                         size_t bank_bytes, void* stream) {
    return olp_push("cp_online_multi_push_proj", false, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples, total_windows,
                    mean_std, OlMap{map_src, map_fill, embeddings, bank}, pred, voted, logits, windows, bank_bytes, stream);
}

extern "C" int cp_online_multi_adapt_push_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                               size_t ws_bytes, const float* raw, const int32_t* counts, int64_t total_samples,
                                               int32_t total_windows, const float* mean_std, const int32_t* map_src,
                                               const float* map_fill, int32_t* pred, int32_t* voted, float* logits, float* windows,
                                               float* embeddings, const void* bank, size_t bank_bytes, void* stream) {
    return olp_push("cp_online_multi_adapt_push_proj", true, cfg, n_streams, max_rows, ws, ws_bytes, raw, counts, total_samples,
                    total_windows, mean_std, OlMap{map_src, map_fill, embeddings, bank}, pred, voted, logits, windows, bank_bytes, stream);
}

// what the enrolment and sweep entries with a bank check of their workspace: the form's view of stream `index` (the folded form:
// its class table; the weights are shared) and, with a bank, the stream's slot
static int olp_check_stream(const char* who, bool adaptive, const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                            size_t ws_bytes, int32_t index, const void* bank, size_t bank_bytes, OlWS* w, const void** own_slot) {
    if (int e = olm_check(cfg, n_streams, max_rows, ws, ws_bytes, adaptive, w)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if (bank)
        if (int e = olp_check_bank(who, cfg->dtype, bank, bank_bytes, n_streams)) return e;
    if (adaptive) *w = ol_stream(*w, index);
    else w->state += (size_t)index * sizeof(OlState);
    *own_slot = bank ? (const unsigned char*)bank + (size_t)index * olp_bank_bytes(1, cfg->dtype) : nullptr;
    return 0;
}

static int olp_enroll(const char* who, bool adaptive, const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                      size_t ws_bytes, int32_t index, const void* bank, size_t bank_bytes, const float* windows, int64_t n_windows,
                      const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes, void* stream) {
    OlWS view;
    const void* own = nullptr;
    if (int e = olp_check_stream(who, adaptive, cfg, n_streams, max_rows, ws, ws_bytes, index, bank, bank_bytes, &view, &own)) return e;
    return ole_enroll(who, cfg, [&](OlWS* w) { *w = view; return 0; }, adaptive, ws, windows, n_windows, slots, n_classes, acc, scratch,
                      scratch_bytes, stream, own);
}

extern "C" int cp_online_multi_enroll_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                           int32_t index, const void* bank, size_t bank_bytes, const float* windows, int64_t n_windows,
                                           const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes,
                                           void* stream) {
    return olp_enroll("cp_online_multi_enroll_proj", false, cfg, n_streams, max_rows, ws, ws_bytes, index, bank, bank_bytes, windows,
                      n_windows, slots, n_classes, acc, scratch, scratch_bytes, stream);
}

extern "C" int cp_online_multi_adapt_enroll_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                 size_t ws_bytes, int32_t index, const void* bank, size_t bank_bytes, const float* windows,
                                                 int64_t n_windows, const int32_t* slots, int32_t n_classes, double* acc, void* scratch,
                                                 size_t scratch_bytes, void* stream) {
    return olp_enroll("cp_online_multi_adapt_enroll_proj", true, cfg, n_streams, max_rows, ws, ws_bytes, index, bank, bank_bytes, windows,
                      n_windows, slots, n_classes, acc, scratch, scratch_bytes, stream);
}

static int olp_map_sweep(const char* who, bool adaptive, const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                         size_t ws_bytes, int32_t index, const void* bank, size_t bank_bytes, OlMapSweep a, void* stream) {
    OlWS view;
    if (int e = olp_check_stream(who, adaptive, cfg, n_streams, max_rows, ws, ws_bytes, index, bank, bank_bytes, &view, &a.own_slot)) return e;
    return olmap_sweep(who, cfg, [&](OlWS* w) { *w = view; return 0; }, adaptive, ws, a, stream);
}

extern "C" int cp_online_multi_map_sweep_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                              int32_t index, const void* bank, size_t bank_bytes, const float* rms, int64_t n_windows,
                                              const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps,
                                              int32_t n_classes, const int32_t* expected_slot, int64_t chunk_rows, void* scratch,
                                              size_t scratch_bytes, int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits,
                                              void* stream) {
    const OlMapSweep a{rms, n_windows, mean_std, map_src, map_fill, n_maps, n_classes, expected_slot, chunk_rows, scratch, scratch_bytes,
                       pred, voted, scores, class_hits, nullptr};
    return olp_map_sweep("cp_online_multi_map_sweep_proj", false, cfg, n_streams, max_rows, ws, ws_bytes, index, bank, bank_bytes, a, stream);
}

extern "C" int cp_online_multi_adapt_map_sweep_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                                    size_t ws_bytes, int32_t index, const void* bank, size_t bank_bytes, const float* rms,
                                                    int64_t n_windows, const float* mean_std, const int32_t* map_src,
                                                    const float* map_fill, int32_t n_maps, int32_t n_classes,
                                                    const int32_t* expected_slot, int64_t chunk_rows, void* scratch, size_t scratch_bytes,
                                                    int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits, void* stream) {
    const OlMapSweep a{rms, n_windows, mean_std, map_src, map_fill, n_maps, n_classes, expected_slot, chunk_rows, scratch, scratch_bytes,
                       pred, voted, scores, class_hits, nullptr};
    return olp_map_sweep("cp_online_multi_adapt_map_sweep_proj", true, cfg, n_streams, max_rows, ws, ws_bytes, index, bank, bank_bytes, a,
                         stream);
}

// ---------------------------------------------------------------------------------------
// joint-angle decoding (csrc/online_kinematics.cuh): where a push leaves its tail inputs, the moments of a recording's tail
// inputs against the glove sample of every window, the fitted readouts applied and scored on held-out windows, and one OknState
// per stream in a workspace of its own behind any decoder's push
// ---------------------------------------------------------------------------------------
static_assert(OKN_MAXD == CP_ONLINE_KIN_MAX_JOINTS && OKN_MAXSMOOTH == CP_ONLINE_KIN_MAX_SMOOTH && OKN_ONE == CP_ONLINE_KIN_ONE &&
              OKN_SUMS == CP_ONLINE_KIN_SUMS && OKN_MAXM == CP_ONLINE_MAX_WINDOWS, "kinematics limits");
static_assert(sizeof(OknState) == 4 * (8 + 6 * OKN_MAXD + OKN_MAXSMOOTH * OKN_MAXD + OKN_MAXD * OKN_F) && sizeof(OknState) % 16 == 0 &&
              offsetof(OknState, W) % 16 == 0 && offsetof(OknState, ring) % 16 == 0,
              "OknState is 18632 words (JointAngles.state reads it back)");
static_assert(sizeof(OknScoreArgs) <= 4096 && sizeof(OknModelArgs) <= 4096, "kinematics kernel arguments");

extern "C" size_t cp_online_tail_offset(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, int32_t adaptive, int32_t multi) {
    const char* who = "cp_online_tail_offset";
    auto bad = [&](const char* what) { ol_fail(CP_ERR_ARG, who, what); return (size_t)0; };
    if (!cfg) return bad("config is required");
    if (cfg->dtype != CP_F32 && cfg->dtype != CP_BF16) return bad("dtype must be CP_F32 or CP_BF16 (no 8-bit path)");
    if (cfg->max_windows < 1 || cfg->max_windows > CP_ONLINE_MAX_WINDOWS) return bad("max_windows outside 1..256");
    if (multi) {
        if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
        if (max_rows < 1 || max_rows > CP_ONLINE_MULTI_MAX_ROWS) return bad("max_rows outside 1..65536");
        return ol_carve(max_rows, cfg->dtype, n_streams, adaptive != 0, true).H1;
    }
    if (n_streams != 1) return bad("a single-stream form has one stream");
    return ol_carve(cfg->max_windows, cfg->dtype, 1, adaptive != 0, false).H1;
}

extern "C" int cp_online_kin_moments(const void* u, int32_t dtype, int64_t n_rows, const int32_t* group, const double* weight,
                                     const float* y, int32_t ldy, int32_t n_joints, int32_t n_groups, double* G, double* C,
                                     void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_kin_moments";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (dtype != CP_F32 && dtype != CP_BF16) return bad("dtype must be CP_F32 or CP_BF16");
    if (n_rows < 0 || n_rows > (int64_t)1 << 24) return bad("n_rows outside 0..2**24");
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return bad("n_joints outside 1..32");
    if (n_groups < 1 || n_groups > CP_ONLINE_READOUT_MAX_GROUPS) return bad("n_groups outside 1..16");
    if (ldy < n_joints) return bad("ldy must be at least n_joints");
    if (!G || !C || !scratch) return bad("G, C and scratch are required");
    if (n_rows > 0 && (!u || !group || !weight || !y)) return bad("u, group, weight and y are required");
    if ((uintptr_t)u % 16 || (uintptr_t)group % 4 || (uintptr_t)weight % 8 || (uintptr_t)y % 4 || (uintptr_t)G % 8 || (uintptr_t)C % 8 ||
        (uintptr_t)scratch % 256)
        return bad("misaligned argument");
    if (scratch_bytes < olr_moments_bytes(n_rows < 1 ? 1 : n_rows, n_groups)) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    int32_t* idx = (int32_t*)scratch;
    int32_t* count = (int32_t*)((unsigned char*)scratch + align256((size_t)n_groups * (size_t)(n_rows < 1 ? 1 : n_rows) * 4));
    hipLaunchKernelGGL(okn_index_kernel, dim3(n_groups), dim3(64), 0, (hipStream_t)stream, group, (int)n_rows, idx, count);
    CKL("okn_index_kernel");
    return ol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        OknMomentsArgs<T> a{};
        a.u = (const T*)u; a.weight = weight; a.y = y; a.idx = idx; a.count = count; a.G = G; a.C = C;
        a.n_rows = (int)n_rows; a.ldy = ldy; a.D = n_joints; a.n_groups = n_groups;
        hipLaunchKernelGGL((okn_moments_kernel<T>), dim3(OLR_TILES, n_groups), dim3(OLR_MOM_THREADS), 0, (hipStream_t)stream, a);
        CKL("okn_moments_kernel");
        return 0;
    });
}

extern "C" int cp_online_kin_apply(const void* u, int32_t dtype, int64_t n_rows, const float* W, const float* b, int32_t n_plans,
                                   int32_t n_joints, float* out, void* stream) {
    const char* who = "cp_online_kin_apply";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (dtype != CP_F32 && dtype != CP_BF16) return bad("dtype must be CP_F32 or CP_BF16");
    if (n_rows < 0 || n_rows > (int64_t)1 << 24) return bad("n_rows outside 0..2**24");
    if (n_plans < 0 || n_plans > CP_ONLINE_READOUT_MAX_PLANS) return bad("n_plans outside 0..256");
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return bad("n_joints outside 1..32");
    if (n_rows == 0 || n_plans == 0) return 0;
    if (!u || !W || !b || !out) return bad("u, W, b and out are required");
    if ((uintptr_t)u % 16 || (uintptr_t)W % 16 || (uintptr_t)b % 4 || (uintptr_t)out % 4) return bad("misaligned argument");
    OknApplyArgs a{};
    a.u = u; a.W = W; a.b = b; a.out = out; a.n_rows = (int)n_rows; a.D = n_joints;
    return ol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((okn_apply_kernel<T>), dim3((unsigned)((n_rows + OKN_BATCH - 1) / OKN_BATCH), n_plans), dim3(OKN_THREADS),
                           OKN_APPLY_LDS, (hipStream_t)stream, a);
        CKL("okn_apply_kernel");
        return 0;
    });
}

extern "C" int cp_online_kin_score(const float* pred, const float* y, int32_t ldy, const int32_t* group, const uint32_t* test_masks,
                                   int32_t n_plans, int64_t n_rows, int32_t n_joints, double* sums, void* stream) {
    const char* who = "cp_online_kin_score";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_rows < 0 || n_rows > (int64_t)1 << 24) return bad("n_rows outside 0..2**24");
    if (n_plans < 0 || n_plans > CP_ONLINE_READOUT_MAX_PLANS) return bad("n_plans outside 0..256");
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return bad("n_joints outside 1..32");
    if (ldy < n_joints) return bad("ldy must be at least n_joints");
    if (n_plans == 0) return 0;
    if (!test_masks || !sums) return bad("test_masks and sums are required");
    if (n_rows > 0 && (!pred || !y || !group)) return bad("pred, y and group are required");
    if ((uintptr_t)pred % 4 || (uintptr_t)y % 4 || (uintptr_t)group % 4 || (uintptr_t)sums % 8) return bad("misaligned argument");
    OknScoreArgs a{};
    for (int t = 0; t < n_plans; ++t) {
        if (test_masks[t] >> CP_ONLINE_READOUT_MAX_GROUPS) return bad("a plan's test mask names a group at or above 16");
        a.mask[t] = (unsigned short)test_masks[t];
    }
    a.pred = pred; a.y = y; a.group = group; a.sums = sums; a.n_rows = (int)n_rows; a.ldy = ldy; a.D = n_joints;
    hipLaunchKernelGGL(okn_score_kernel, dim3(n_plans), dim3(64), 0, (hipStream_t)stream, a);
    CKL("okn_score_kernel");
    return 0;
}

static int okn_check(const char* who, const cp_online_kin_config* c, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!c || !ws) return bad("config and workspace are required");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if (c->smooth < 1 || c->smooth > CP_ONLINE_KIN_MAX_SMOOTH) return bad("smooth outside 1..64");
    if (c->rate < 1 || c->rate > CP_ONLINE_KIN_ONE) return bad("rate outside 1..4096");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes < (size_t)n_streams * sizeof(OknState)) return ol_fail(CP_ERR_WORKSPACE, who, "workspace too small");
    return 0;
}

extern "C" size_t cp_online_kin_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(OknState));
}

extern "C" int cp_online_kin_set_model(const cp_online_kin_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                       const float* W, const float* b, int32_t n_joints, const float* lo, const float* span,
                                       const int32_t* rest, void* stream) {
    const char* who = "cp_online_kin_set_model";
    if (int e = okn_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return ol_fail(CP_ERR_ARG, who, "n_joints outside 1..32");
    if (!W || !b || !lo || !span || !rest) return ol_fail(CP_ERR_ARG, who, "W, b, lo, span and rest are required");
    if ((uintptr_t)W % 16 || (uintptr_t)b % 4) return ol_fail(CP_ERR_ARG, who, "misaligned W or b");
    OknModelArgs p{};
    p.D = n_joints;
    for (int d = 0; d < n_joints; ++d) {
        if (!std::isfinite(lo[d])) return ol_fail(CP_ERR_ARG, who, "lo must be finite");
        if (!(span[d] > 0.f) || !std::isfinite(span[d])) return ol_fail(CP_ERR_ARG, who, "span must be finite and > 0");
        if (rest[d] < 0 || rest[d] > CP_ONLINE_KIN_ONE) return ol_fail(CP_ERR_ARG, who, "rest outside 0..4096");
        p.lo[d] = lo[d];
        p.span[d] = span[d];
        p.rest[d] = rest[d];
    }
    hipLaunchKernelGGL(okn_set_model_kernel, dim3(1), dim3(OKN_THREADS), 0, (hipStream_t)stream, (OknState*)ws + index, W, b, p);
    CKL("okn_set_model_kernel");
    return 0;
}

extern "C" int cp_online_kin_reset(const cp_online_kin_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                   void* stream) {
    const char* who = "cp_online_kin_reset";
    if (int e = okn_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return ol_fail(CP_ERR_ARG, who, "stream index outside -1..n_streams-1");
    hipLaunchKernelGGL(okn_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(OKN_THREADS), 0, (hipStream_t)stream, (OknState*)ws,
                       index < 0 ? 0 : index);
    CKL("okn_reset_kernel");
    return 0;
}

// more than 64 KB of dynamic LDS needs the opt-in once per process and kernel
template <typename T>
static int okn_push_launch(int32_t n_streams, const OknPushArgs& a, void* stream) {
    static bool attr_set = false;
    if (!attr_set) {
        CK(hipFuncSetAttribute((const void*)okn_push_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, OKN_PUSH_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL((okn_push_kernel<T>), dim3(n_streams), dim3(OKN_THREADS), OKN_PUSH_LDS, (hipStream_t)stream, a);
    CKL("okn_push_kernel");
    return 0;
}

extern "C" int cp_online_kin_push(const cp_online_kin_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const void* tail,
                                  int32_t dtype, int32_t ldt, const int32_t* cls, const int32_t* row0, const int32_t* m,
                                  int32_t total_rows, float* raw, int32_t* pose, float* angle, void* stream) {
    const char* who = "cp_online_kin_push";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (int e = okn_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (dtype != CP_F32 && dtype != CP_BF16) return bad("dtype must be CP_F32 or CP_BF16");
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return bad("total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (ldt < OKN_F) return bad("ldt must be at least 512");
    if (!tail || !row0 || !m || !raw || !pose || !angle) return bad("tail, row0, m, raw, pose and angle are required");
    const size_t es = dtype == CP_BF16 ? 2 : 4;
    if ((uintptr_t)tail % 16 || ((size_t)ldt * es) % 16 || (uintptr_t)cls % 4 || (uintptr_t)row0 % 4 || (uintptr_t)m % 4 ||
        (uintptr_t)raw % 4 || (uintptr_t)pose % 4 || (uintptr_t)angle % 4)
        return bad("misaligned argument");
    OknPushArgs a{};
    a.states = (OknState*)ws; a.tail = tail; a.cls = cls; a.row0 = row0; a.m = m; a.ldt = ldt; a.total_rows = total_rows;
    a.smooth = cfg->smooth; a.rate = cfg->rate; a.raw = raw; a.pose = pose; a.angle = angle;
    return ol_dispatch(dtype, [&](auto t) { return okn_push_launch<decltype(t)>(n_streams, a, stream); });
}

// ---------------------------------------------------------------------------------------
// pose filter (csrc/online_kalman.cuh): the trajectory and error moments of a cued recording, the steady-state gain of every
// plan, the held-out sweep, and one OkfState per stream in a workspace of its own behind any decoder's push
// ---------------------------------------------------------------------------------------
static_assert(OKF_MAX_ITERS == CP_ONLINE_KF_MAX_ITERS && OKF_SUMS == CP_ONLINE_KF_SUMS && OKF_MAXD == CP_ONLINE_KIN_MAX_JOINTS,
              "pose filter limits");
static_assert(sizeof(OkfState) == 4 * (8 + OKF_MAXS + 6 * OKF_MAXD + OKF_MAXS * OKF_MAXS + OKF_MAXS * OKF_MAXD + OKF_MAXD * OKN_F) &&
              sizeof(OkfState) % 16 == 0 && offsetof(OkfState, M) % 16 == 0 && offsetof(OkfState, W) % 16 == 0 &&
              offsetof(OkfState, K) == offsetof(OkfState, M) + sizeof(float) * OKF_MAXS * OKF_MAXS,
              "OkfState is 22792 words (PoseFilter.state reads it back)");
static_assert(sizeof(OkfDesignArgs) <= 4096 && sizeof(OkfSweepArgs) <= 4096 && sizeof(OkfMomentsArgs) <= 4096 && sizeof(OkfModelArgs) <= 4096,
              "pose filter kernel arguments");

static int okf_check_centre(const char* who, const float* centre, int32_t n_joints, float* out) {
    if (!centre) return ol_fail(CP_ERR_ARG, who, "centre is required");
    for (int d = 0; d < n_joints; ++d) {
        if (!std::isfinite(centre[d])) return ol_fail(CP_ERR_ARG, who, "centre must be finite");
        out[d] = centre[d];
    }
    return 0;
}

extern "C" int cp_online_kf_moments(const float* a, const float* y, const int32_t* group, int64_t n_rows, int32_t n_joints,
                                    int32_t n_groups, const float* centre, double* G, double* C, double* S, double* E, int32_t* count,
                                    void* stream) {
    const char* who = "cp_online_kf_moments";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_rows < 0 || n_rows > (int64_t)1 << 24) return bad("n_rows outside 0..2**24");
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return bad("n_joints outside 1..32");
    if (n_groups < 1 || n_groups > CP_ONLINE_READOUT_MAX_GROUPS) return bad("n_groups outside 1..16");
    if (!G || !C || !S || !E || !count) return bad("G, C, S, E and count are required");
    if (n_rows > 0 && (!a || !y || !group)) return bad("a, y and group are required");
    if ((uintptr_t)a % 4 || (uintptr_t)y % 4 || (uintptr_t)group % 4 || (uintptr_t)G % 8 || (uintptr_t)C % 8 || (uintptr_t)S % 8 ||
        (uintptr_t)E % 8 || (uintptr_t)count % 4)
        return bad("misaligned argument");
    OkfMomentsArgs k{};
    if (int e = okf_check_centre(who, centre, n_joints, k.c)) return e;
    k.a = a; k.y = y; k.group = group; k.G = G; k.C = C; k.S = S; k.E = E; k.count = count; k.n_rows = (int)n_rows; k.D = n_joints;
    hipLaunchKernelGGL(okf_moments_kernel, dim3(n_groups), dim3(OKF_THREADS), 0, (hipStream_t)stream, k);
    CKL("okf_moments_kernel");
    return 0;
}

extern "C" size_t cp_online_kf_design_bytes(int32_t n_plans) {
    if (n_plans < 1) n_plans = 1;
    if (n_plans > OKF_PLANS_PER_LAUNCH) n_plans = OKF_PLANS_PER_LAUNCH;
    return align256((size_t)n_plans * OKF_PLAN_DOUBLES * sizeof(double));
}

extern "C" int cp_online_kf_design(const double* G, const double* C, const double* S, const double* E, const int32_t* count,
                                   int32_t n_joints, int32_t n_groups, const cp_online_kf_plan* plans, int32_t n_plans, float* M,
                                   float* K, double* delta, int32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "cp_online_kf_design";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return bad("n_joints outside 1..32");
    if (n_groups < 1 || n_groups > CP_ONLINE_READOUT_MAX_GROUPS) return bad("n_groups outside 1..16");
    if (n_plans < 0 || n_plans > CP_ONLINE_READOUT_MAX_PLANS) return bad("n_plans outside 0..256");
    if (n_plans == 0) return 0;
    if (!G || !C || !S || !E || !count || !plans || !M || !K || !delta || !status || !scratch)
        return bad("G, C, S, E, count, plans, M, K, delta, status and scratch are required");
    if ((uintptr_t)G % 8 || (uintptr_t)C % 8 || (uintptr_t)S % 8 || (uintptr_t)E % 8 || (uintptr_t)count % 4 || (uintptr_t)M % 4 ||
        (uintptr_t)K % 4 || (uintptr_t)delta % 8 || (uintptr_t)status % 4 || (uintptr_t)scratch % 256)
        return bad("misaligned argument");
    for (int t = 0; t < n_plans; ++t) {
        const cp_online_kf_plan& p = plans[t];
        if (p.groups >> n_groups) return bad("a plan's mask names a group at or above n_groups");
        if (p.iters < 1 || p.iters > CP_ONLINE_KF_MAX_ITERS) return bad("a plan's iters outside 1..1024");
        if (!(p.lam >= 0.0) || !std::isfinite(p.lam)) return bad("a plan's lam must be finite and >= 0");
        if (!(p.rho > 0.0) || !std::isfinite(p.rho)) return bad("a plan's rho must be finite and > 0");
        if (!(p.kappa > 0.0) || !std::isfinite(p.kappa)) return bad("a plan's kappa must be finite and > 0");
    }
    if (scratch_bytes < cp_online_kf_design_bytes(n_plans)) return ol_fail(CP_ERR_WORKSPACE, who, "scratch too small");
    static bool attr_set = false;
    if (!attr_set) {                                           // more than 64 KB of dynamic LDS needs the opt-in once per process
        CK(hipFuncSetAttribute((const void*)okf_design_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, OKF_DESIGN_LDS));
        attr_set = true;
    }
    const int n2 = 2 * n_joints;
    for (int t0 = 0; t0 < n_plans; t0 += OKF_PLANS_PER_LAUNCH) {
        const int np = n_plans - t0 < OKF_PLANS_PER_LAUNCH ? n_plans - t0 : OKF_PLANS_PER_LAUNCH;
        OkfDesignArgs k{};
        k.G = G; k.C = C; k.S = S; k.E = E; k.count = count; k.scratch = (double*)scratch; k.D = n_joints; k.n_groups = n_groups;
        k.M = M + (size_t)t0 * n2 * n2; k.K = K + (size_t)t0 * n2 * n_joints; k.delta = delta + t0; k.status = status + t0;
        for (int t = 0; t < np; ++t) {
            const cp_online_kf_plan& p = plans[t0 + t];
            k.mask[t] = (unsigned short)p.groups; k.iters[t] = (unsigned short)p.iters; k.lam[t] = p.lam; k.rho[t] = p.rho; k.kappa[t] = p.kappa;
        }
        hipLaunchKernelGGL(okf_design_kernel, dim3(np), dim3(OKF_THREADS), (size_t)okf_design_doubles(n_joints) * 8, (hipStream_t)stream, k);
        CKL("okf_design_kernel");
    }
    return 0;
}

extern "C" int cp_online_kf_sweep(const float* a, const float* y, const int32_t* group, int64_t n_rows, int32_t n_joints,
                                  const uint32_t* test_masks, int32_t n_plans, const float* M, const float* K, const float* centre,
                                  double* sums, float* filtered, void* stream) {
    const char* who = "cp_online_kf_sweep";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (n_rows < 0 || n_rows > (int64_t)1 << 24) return bad("n_rows outside 0..2**24");
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return bad("n_joints outside 1..32");
    if (n_plans < 0 || n_plans > CP_ONLINE_READOUT_MAX_PLANS) return bad("n_plans outside 0..256");
    if (n_plans == 0) return 0;
    if (!test_masks || !M || !K || !sums) return bad("test_masks, M, K and sums are required");
    if (n_rows > 0 && (!a || !y || !group)) return bad("a, y and group are required");
    if ((uintptr_t)a % 4 || (uintptr_t)y % 4 || (uintptr_t)group % 4 || (uintptr_t)M % 4 || (uintptr_t)K % 4 || (uintptr_t)sums % 8 ||
        (uintptr_t)filtered % 4)
        return bad("misaligned argument");
    OkfSweepArgs k{};
    if (int e = okf_check_centre(who, centre, n_joints, k.c)) return e;
    for (int t = 0; t < n_plans; ++t) {
        if (test_masks[t] >> CP_ONLINE_READOUT_MAX_GROUPS) return bad("a plan's test mask names a group at or above 16");
        k.mask[t] = (unsigned short)test_masks[t];
    }
    k.a = a; k.y = y; k.group = group; k.M = M; k.K = K; k.sums = sums; k.filtered = filtered; k.n_rows = (int)n_rows; k.D = n_joints;
    hipLaunchKernelGGL(okf_sweep_kernel, dim3(n_plans), dim3(64), 0, (hipStream_t)stream, k);
    CKL("okf_sweep_kernel");
    return 0;
}

static int okf_check(const char* who, const cp_online_kf_config* c, int32_t n_streams, void* ws, size_t ws_bytes) {
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (!c || !ws) return bad("config and workspace are required");
    if (n_streams < 1 || n_streams > CP_ONLINE_MULTI_MAX_STREAMS) return bad("n_streams outside 1..256");
    if (c->rate < 1 || c->rate > CP_ONLINE_KIN_ONE) return bad("rate outside 1..4096");
    if ((uintptr_t)ws % 256) return bad("workspace not 256-byte aligned");
    if (ws_bytes < (size_t)n_streams * sizeof(OkfState)) return ol_fail(CP_ERR_WORKSPACE, who, "workspace too small");
    return 0;
}

extern "C" size_t cp_online_kf_workspace_bytes(int32_t n_streams) {
    if (n_streams < 1) n_streams = 1;
    return align256((size_t)n_streams * sizeof(OkfState));
}

extern "C" int cp_online_kf_set_model(const cp_online_kf_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                      const float* W, const float* b, int32_t n_joints, const float* lo, const float* span,
                                      const int32_t* rest, const float* M, const float* K, void* stream) {
    const char* who = "cp_online_kf_set_model";
    if (int e = okf_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (int e = ol_check_index(who, index, n_streams)) return e;
    if (n_joints < 1 || n_joints > CP_ONLINE_KIN_MAX_JOINTS) return ol_fail(CP_ERR_ARG, who, "n_joints outside 1..32");
    if (!W || !b || !lo || !span || !rest || !M || !K) return ol_fail(CP_ERR_ARG, who, "W, b, lo, span, rest, M and K are required");
    if ((uintptr_t)W % 16 || (uintptr_t)b % 4 || (uintptr_t)M % 4 || (uintptr_t)K % 4) return ol_fail(CP_ERR_ARG, who, "misaligned W, b, M or K");
    OkfModelArgs p{};
    p.D = n_joints;
    for (int d = 0; d < n_joints; ++d) {
        if (!std::isfinite(lo[d])) return ol_fail(CP_ERR_ARG, who, "lo must be finite");
        if (!(span[d] > 0.f) || !std::isfinite(span[d])) return ol_fail(CP_ERR_ARG, who, "span must be finite and > 0");
        if (rest[d] < 0 || rest[d] > CP_ONLINE_KIN_ONE) return ol_fail(CP_ERR_ARG, who, "rest outside 0..4096");
        p.lo[d] = lo[d];
        p.span[d] = span[d];
        p.rest[d] = rest[d];
    }
    hipLaunchKernelGGL(okf_set_model_kernel, dim3(1), dim3(OKF_THREADS), 0, (hipStream_t)stream, (OkfState*)ws + index, W, b, M, K, p);
    CKL("okf_set_model_kernel");
    return 0;
}

extern "C" int cp_online_kf_reset(const cp_online_kf_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream) {
    const char* who = "cp_online_kf_reset";
    if (int e = okf_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (index < -1 || index >= n_streams) return ol_fail(CP_ERR_ARG, who, "stream index outside -1..n_streams-1");
    hipLaunchKernelGGL(okf_reset_kernel, dim3(index < 0 ? n_streams : 1), dim3(OKF_THREADS), 0, (hipStream_t)stream, (OkfState*)ws,
                       index < 0 ? 0 : index);
    CKL("okf_reset_kernel");
    return 0;
}

template <typename T>
static int okf_push_launch(int32_t n_streams, const OkfPushArgs& a, void* stream) {
    static bool attr_set = false;
    if (!attr_set) {                                           // more than 64 KB of dynamic LDS needs the opt-in once per process and kernel
        CK(hipFuncSetAttribute((const void*)okf_push_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, OKF_PUSH_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL((okf_push_kernel<T>), dim3(n_streams), dim3(OKF_THREADS), OKF_PUSH_LDS, (hipStream_t)stream, a);
    CKL("okf_push_kernel");
    return 0;
}

extern "C" int cp_online_kf_push(const cp_online_kf_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const void* tail,
                                 int32_t dtype, int32_t ldt, const int32_t* cls, const int32_t* row0, const int32_t* m,
                                 int32_t total_rows, float* raw, float* filtered, int32_t* pose, float* angle, void* stream) {
    const char* who = "cp_online_kf_push";
    auto bad = [&](const char* what) { return ol_fail(CP_ERR_ARG, who, what); };
    if (int e = okf_check(who, cfg, n_streams, ws, ws_bytes)) return e;
    if (dtype != CP_F32 && dtype != CP_BF16) return bad("dtype must be CP_F32 or CP_BF16");
    if (total_rows < 0 || total_rows > CP_ONLINE_MULTI_MAX_ROWS) return bad("total_rows outside 0..65536");
    if (total_rows == 0) return 0;
    if (ldt < OKN_F) return bad("ldt must be at least 512");
    if (!tail || !row0 || !m || !raw || !filtered || !pose || !angle) return bad("tail, row0, m, raw, filtered, pose and angle are required");
    const size_t es = dtype == CP_BF16 ? 2 : 4;
    if ((uintptr_t)tail % 16 || ((size_t)ldt * es) % 16 || (uintptr_t)cls % 4 || (uintptr_t)row0 % 4 || (uintptr_t)m % 4 ||
        (uintptr_t)raw % 4 || (uintptr_t)filtered % 4 || (uintptr_t)pose % 4 || (uintptr_t)angle % 4)
        return bad("misaligned argument");
    OkfPushArgs a{};
    a.states = (OkfState*)ws; a.tail = tail; a.cls = cls; a.row0 = row0; a.m = m; a.ldt = ldt; a.total_rows = total_rows;
    a.rate = cfg->rate; a.raw = raw; a.filtered = filtered; a.pose = pose; a.angle = angle;
    return ol_dispatch(dtype, [&](auto t) { return okf_push_launch<decltype(t)>(n_streams, a, stream); });
}
