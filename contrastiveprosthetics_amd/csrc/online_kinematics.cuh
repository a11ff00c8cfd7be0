// Joint-angle decoding (include/cpnative.h, cp_online_kin_*): a ridge pose readout behind the decoders.  The tail inputs u of a
// recording (cp_online_*tail_inputs) are regressed onto the glove sample of every window, x = [u, 1] (513 values), up to
// OKN_MAXD joints; the fitted W (D x 512) and b (D) then turn the tail inputs every push leaves in its workspace
// (cp_online_tail_offset) into a bounded, smoothed, rate-limited pose per window and stream.  The numpy definitions are in
// contrastiveprosthetics_amd/kinematics.py (moments_reference, pose_reference, JointReference, score_reference); every kernel
// here equals them in every bit.  The normal equations are solved by cp_online_readout_solve, 16 joints at a time.
//
//   okn_index_kernel     grid n_groups, one wave per group: the windows of the group in window order (olr_index_kernel without a
//                        slot).
//   okn_moments_kernel   grid (45 tiles, n_groups), olr_moments_kernel's shape with the window's own target row in place of a
//                        class row: the extended row x~ = [u (512), 1, y (32)] has 545 entries, the lower triangle of
//                        sum w x~ x~^T in 64 x 64 tiles holds G (rows and columns < 513) and C (rows 513..544, columns < 513).
//                        Windows are staged OLR_STAGE at a time in LDS; per window and element p = x_a * x_b (exact in f64),
//                        q = w * p, acc = acc + q, each rounded on its own, in window order: no slabs, no atomics.  C leaves
//                        in column blocks of 16, (2, n_groups, 513, 16), the layout cp_online_readout_solve takes.
//   okn_pose_row         the pose matvec of one row on one wave (device function; the apply and the stage both call it): lane l
//                        sums the products W[d][l + 64 j] * u[l + 64 j], j = 0..7 ascending, from +0.0f, then the 64 partial
//                        sums fold as p[l] += p[l + s], s = 32, 16, .., 1, then + b[d]; single f32 operations, no contraction.
//   okn_apply_kernel     grid (chunks of OKN_BATCH rows, plans), four waves; the plan's W is staged in LDS once.
//   okn_score_kernel     grid n_plans, one wave per plan, lane = joint: the seven f64 sums over the plan's held-out windows in
//                        window order.
//   okn_push_kernel      grid n_streams, four waves per stream, one launch per push.  The stream's W (at most 64 KB) and ring
//                        are staged in LDS once; the stream's rows are taken OKN_BATCH at a time: the four waves share the
//                        rows of the batch for the matvec (row j to wave j % 4), then wave 0 runs the state machine over the
//                        batch in window order, lane = joint.  A stream without rows, without a model or with rows outside the
//                        launch is left untouched.
//   okn_set_model_kernel, okn_reset_kernel   one workgroup per stream.
// Everything is integer or single f32 / f64 operations with floating-point contraction off and plain vector stores: no
// floating-point atomics, no grid-wide barrier, no persistent kernel.  The outputs are the same for any cutting of a stream's
// rows into calls and for any set of streams that share a launch.
#pragma once
#include "online_readout.cuh"

constexpr int OKN_MAXD = 32;                     // joints (CP_ONLINE_KIN_MAX_JOINTS)
constexpr int OKN_F = 512;                       // tail inputs per window
constexpr int OKN_MAXSMOOTH = 64;                // ring length (CP_ONLINE_KIN_MAX_SMOOTH)
constexpr int OKN_ONE = 4096;                    // full level (CP_ONLINE_KIN_ONE)
constexpr int OKN_MAXM = 256;                    // rows of one stream per push (CP_ONLINE_MAX_WINDOWS)
constexpr int OKN_THREADS = 256;                 // four waves
constexpr int OKN_BATCH = 64;                    // rows of a stream (stage) or of a chunk (apply) between two barriers
constexpr int OKN_JU = 4;                        // joints whose partial sums the matvec folds side by side
constexpr int OKN_SUMS = 7;                     // n, sum y, sum y^2, sum p, sum p^2, sum y p, sum (p - y)^2
constexpr int OKN_E = OLR_X + OKN_MAXD;          // x~ = [u, 1, y]: 545
constexpr int OKN_APPLY_LDS = OKN_MAXD * OKN_F * 4;                                    // a plan's W
constexpr int OKN_PUSH_LDS = OKN_APPLY_LDS + OKN_BATCH * OKN_MAXD * 4 + OKN_MAXSMOOTH * OKN_MAXD * 4;   // W, the batch's a, the ring
static_assert((OKN_E + OLR_TILE - 1) / OLR_TILE == OLR_NT && OKN_MAXD == 2 * CP_D_E && OKN_F == OLR_F, "kinematics layout");

// ---------------------------------------------------------------------------------------
// moments
// ---------------------------------------------------------------------------------------
// grid n_groups, 64 threads: idx[r][0..count[r]) = the windows w with group[w] == r, ascending
__global__ __launch_bounds__(64) void okn_index_kernel(const int32_t* __restrict__ group, int n_rows, int32_t* __restrict__ idx,
                                                       int32_t* __restrict__ count) {
    const int lane = threadIdx.x, r = blockIdx.x;
    int32_t* out = idx + (size_t)r * n_rows;
    int n = 0;
    for (int base = 0; base < n_rows; base += 64) {
        const int w = base + lane;
        const bool mine = w < n_rows && group[w] == r;
        const unsigned long long m = __ballot(mine);
        if (mine) out[n + __popcll(m & ((1ull << lane) - 1ull))] = w;
        n += __popcll(m);
    }
    if (lane == 0) count[r] = n;
}

template <typename T>
struct OknMomentsArgs {
    const T* u;                          // [n_rows][512]
    const double* weight;                // [n_rows]
    const float* y;                      // [n_rows][ldy], D columns in use
    const int32_t* idx;                  // [n_groups][n_rows]
    const int32_t* count;                // [n_groups]
    double* G;                           // [n_groups][513][513], symmetric
    double* C;                           // [2][n_groups][513][16]
    int n_rows, ldy, D, n_groups;
};

// entry e of x~ of window w (checked by the caller)
template <typename T>
__device__ __forceinline__ float okn_entry(const OknMomentsArgs<T>& a, int w, int e) {
    if (e < OKN_F) return olf_widen<T>(a.u[(size_t)w * OKN_F + e]);
    if (e == OKN_F) return 1.f;
    if (e < OLR_X + a.D) return a.y[(size_t)w * a.ldy + (e - OLR_X)];
    return 0.f;
}

template <typename T>
__global__ __launch_bounds__(OLR_MOM_THREADS) void okn_moments_kernel(OknMomentsArgs<T> a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float rowv[OLR_STAGE][OLR_TILE];
    __shared__ __attribute__((aligned(16))) float colv[OLR_STAGE][OLR_TILE];
    __shared__ double wv[OLR_STAGE];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, r = blockIdx.y;
    int ti = 0, rem = blockIdx.x;                              // tile (ti, tj), tj <= ti
    while (rem > ti) {
        rem -= ti + 1;
        ++ti;
    }
    const int tj = rem, a0 = ti * OLR_TILE, b0 = tj * OLR_TILE;
    int n = a.count[r];
    n = n < 0 ? 0 : (n > a.n_rows ? a.n_rows : n);
    const int32_t* list = a.idx + (size_t)r * a.n_rows;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int base = 0; base < n; base += OLR_STAGE) {
        const int ns = min(OLR_STAGE, n - base);
        __syncthreads();                                       // the stage before has been read
        for (int e = tid; e < OLR_STAGE * 2 * OLR_TILE; e += OLR_MOM_THREADS) {
            const int s = e / (2 * OLR_TILE), q = e % (2 * OLR_TILE);
            float v = 0.f;
            double om = 0.0;
            if (s < ns) {
                const int w = list[base + s];
                if (w >= 0 && w < a.n_rows) {
                    v = okn_entry<T>(a, w, q < OLR_TILE ? a0 + q : b0 + q - OLR_TILE);
                    om = a.weight[w];
                }
            }
            if (q < OLR_TILE) rowv[s][q] = v;
            else colv[s][q - OLR_TILE] = v;
            if (q == 0) wv[s] = om;
        }
        __syncthreads();
        for (int s = 0; s < ns; ++s) {
            const double om = wv[s];
            const float4 rv = *(const float4*)&rowv[s][ty * 4];
            const float4 cv = *(const float4*)&colv[s][tx * 4];
            const double rd[4] = {(double)rv.x, (double)rv.y, (double)rv.z, (double)rv.w};
            const double cd[4] = {(double)cv.x, (double)cv.y, (double)cv.z, (double)cv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double p = rd[i] * cd[j];            // exact: two f32 values
                    const double q = om * p;
                    acc[i][j] = acc[i][j] + q;
                }
        }
    }
    double* G = a.G + (size_t)r * OLR_X * OLR_X;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ea = a0 + ty * 4 + i, eb = b0 + tx * 4 + j;
            if (eb > ea || eb >= OLR_X || ea >= OKN_E) continue;
            if (ea < OLR_X) {
                G[(size_t)ea * OLR_X + eb] = acc[i][j];
                G[(size_t)eb * OLR_X + ea] = acc[i][j];
            } else {                                           // joint d of column block d / 16; a joint past D: zero
                const int d = ea - OLR_X;
                a.C[(((size_t)(d / CP_D_E) * a.n_groups + r) * OLR_X + eb) * CP_D_E + d % CP_D_E] = d < a.D ? acc[i][j] : 0.0;
            }
        }
}

// ---------------------------------------------------------------------------------------
// the pose matvec
// ---------------------------------------------------------------------------------------
// a[d] = W[d] . u + b[d] of one row, on lane d of the calling wave (0.f on the lanes from D on): the definition's order.
// W: [D][512] f32 (LDS or global), b_lane: b[lane] on the lanes below D, u: the row's 512 tail inputs in T.
template <typename T>
__device__ __forceinline__ float okn_pose_row(const float* __restrict__ W, float b_lane, const T* __restrict__ u, int D, int lane) {
#pragma clang fp contract(off)
    float x[OKN_F / 64];
#pragma unroll
    for (int j = 0; j < OKN_F / 64; ++j) x[j] = olf_widen<T>(u[lane + 64 * j]);
    float mine = 0.f;
    for (int d0 = 0; d0 < D; d0 += OKN_JU) {                   // OKN_JU joints at a time: their fold chains do not depend on each other
        float p[OKN_JU];
#pragma unroll
        for (int q = 0; q < OKN_JU; ++q) {
            const float* w = W + min(d0 + q, D - 1) * OKN_F;   // (past D: joint D - 1 again, not kept)
            p[q] = 0.f;
#pragma unroll
            for (int j = 0; j < OKN_F / 64; ++j) {
                const float t = w[lane + 64 * j] * x[j];
                p[q] = p[q] + t;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
#pragma unroll
            for (int q = 0; q < OKN_JU; ++q) p[q] = p[q] + __shfl_down(p[q], s, 64);   // lanes below s hold p[l] + p[l + s]
#pragma unroll
        for (int q = 0; q < OKN_JU; ++q) {
            const float p0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(p[q])));   // lane 0's bits (every lane of the wave is here)
            if (lane == d0 + q && d0 + q < D) mine = p0 + b_lane;
        }
    }
    return mine;
}

struct OknApplyArgs {
    const void* u;                       // [n_rows][512] in T
    const float* W;                      // [n_plans][D][512]
    const float* b;                      // [n_plans][D]
    float* out;                          // [n_plans][n_rows][D]
    int n_rows, D;
};

// grid (chunks of OKN_BATCH rows, n_plans), OKN_APPLY_LDS bytes of dynamic LDS
template <typename T>
__global__ __launch_bounds__(OKN_THREADS) void okn_apply_kernel(OknApplyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float okn_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.y, D = a.D;
    const float4* W4 = (const float4*)(a.W + (size_t)p * D * OKN_F);
    for (int e = tid; e < D * (OKN_F / 4); e += OKN_THREADS) ((float4*)okn_smem)[e] = W4[e];
    const float b = lane < D ? a.b[p * D + lane] : 0.f;
    __syncthreads();
    const int row_begin = blockIdx.x * OKN_BATCH, row_end = min(a.n_rows, row_begin + OKN_BATCH);
    float* out = a.out + (size_t)p * a.n_rows * D;
    for (int row = row_begin + wave; row < row_end; row += OKN_THREADS / 64) {
        const float v = okn_pose_row<T>(okn_smem, b, (const T*)a.u + (size_t)row * OKN_F, D, lane);
        if (lane < D) out[(size_t)row * D + lane] = v;
    }
}

// ---------------------------------------------------------------------------------------
// held-out score
// ---------------------------------------------------------------------------------------
struct OknScoreArgs {
    const float* pred;                   // [n_plans][n_rows][D]
    const float* y;                      // [n_rows][ldy]
    const int32_t* group;                // [n_rows]
    double* sums;                        // [n_plans][D][7]
    int n_rows, ldy, D;
    unsigned short mask[OLR_MAX_PLANS];  // a plan's test groups
};

// grid n_plans, one wave: lane d walks the rows in order for joint d
__global__ __launch_bounds__(64) void okn_score_kernel(OknScoreArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, p = blockIdx.x, D = a.D;
    if (lane >= D) return;
    const unsigned mask = a.mask[p];
    const float* pred = a.pred + (size_t)p * a.n_rows * D;
    double s[OKN_SUMS];
#pragma unroll
    for (int k = 0; k < OKN_SUMS; ++k) s[k] = 0.0;
    constexpr int U = 8;                                       // rows whose loads are in flight together
    for (int base = 0; base < a.n_rows; base += U) {
        int g[U];
        float yv[U], qv[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = min(base + k, a.n_rows - 1);
            g[k] = a.group[i];
            yv[k] = a.y[(size_t)i * a.ldy + lane];
            qv[k] = pred[(size_t)i * D + lane];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (base + k >= a.n_rows || g[k] < 0 || g[k] >= OLR_MAX_GROUPS || !((mask >> g[k]) & 1u)) continue;
            const double y = (double)yv[k], q = (double)qv[k];
            const double yy = y * y, qq = q * q, yq = y * q, e = q - y;
            const double ee = e * e;
            s[0] = s[0] + 1.0;
            s[1] = s[1] + y;
            s[2] = s[2] + yy;
            s[3] = s[3] + q;
            s[4] = s[4] + qq;
            s[5] = s[5] + yq;
            s[6] = s[6] + ee;
        }
    }
#pragma unroll
    for (int k = 0; k < OKN_SUMS; ++k) a.sums[((size_t)p * D + lane) * OKN_SUMS + k] = s[k];
}

// ---------------------------------------------------------------------------------------
// the stage
// ---------------------------------------------------------------------------------------
// Per-stream state.  A zeroed state is a valid start: no model, empty ring, out = 0.
struct OknState {
    int D;                               // ---- model part (survives a reset); 0: no model
    int head, len;                       // ---- stream part: ring position and fill, shared by the joints
    int pad[5];
    int out[OKN_MAXD];                   // the pose, integers out of 4096
    int sum[OKN_MAXD];                   // the sum of each joint's ring entries
    int rest[OKN_MAXD];                  // ---- model
    float lo[OKN_MAXD], span[OKN_MAXD], b[OKN_MAXD];
    int ring[OKN_MAXSMOOTH * OKN_MAXD];  // [entry][joint]: the last `smooth` q of every joint
    float W[OKN_MAXD * OKN_F];           // [joint][512]
};

struct OknPushArgs {
    OknState* states;
    const void* tail;                    // [total_rows][ldt] in T
    const int32_t* cls;                  // [total_rows] class id or -1, or NULL
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int ldt, total_rows, smooth, rate;
    float* raw;                          // [total_rows][32]
    int32_t* pose;                       // [total_rows][32]
    float* angle;                        // [total_rows][32]
};

template <typename T>
__global__ __launch_bounds__(OKN_THREADS) void okn_push_kernel(OknPushArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float okn_smem[];
    float* sW = okn_smem;                                      // [D][512]
    float* sA = sW + OKN_MAXD * OKN_F;                         // [OKN_BATCH][32]: a of the batch's rows
    int* sR = (int*)(sA + OKN_BATCH * OKN_MAXD);               // [smooth][32]
    OknState* st = a.states + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, jl = lane & (OKN_MAXD - 1);
    const int D = st->D, M = a.m[blockIdx.x], r0 = a.row0[blockIdx.x], V = a.smooth, rate = a.rate;
    // a stream without a model, or whose rows disagree with the limits, is left untouched (uniform over the workgroup)
    if (D < 1 || D > OKN_MAXD || M < 1 || M > OKN_MAXM || r0 < 0 || r0 > a.total_rows - M || V < 1 || V > OKN_MAXSMOOTH || rate < 1 ||
        rate > OKN_ONE || a.ldt < OKN_F)
        return;

    // ---- W, the ring and the per-joint values: every load is issued before the first one is waited for
    {
        const float4* W4 = (const float4*)st->W;
        const int4* R4 = (const int4*)st->ring;
        for (int e = tid; e < D * (OKN_F / 4); e += OKN_THREADS) ((float4*)sW)[e] = W4[e];
        for (int e = tid; e < OKN_MAXSMOOTH * OKN_MAXD / 4; e += OKN_THREADS) ((int4*)sR)[e] = R4[e];
    }
    const bool joint = lane < D;                               // (the state machine: lanes 0..D-1 of wave 0)
    const float b = st->b[jl], lo = st->lo[jl], span = st->span[jl];
    const int rest = st->rest[jl];
    int out = st->out[jl], sum = st->sum[jl], head = st->head, len = st->len;
    if (head < 0 || head >= V || len < 0 || len > V) {         // a ring kept under another smooth length: start empty
        head = 0;
        len = 0;
        sum = 0;
    }
    __syncthreads();

    for (int base = 0; base < M; base += OKN_BATCH) {
        const int nb = min(OKN_BATCH, M - base);
        // ---- the matvec: row j of the batch on wave j % 4
        for (int j = wave; j < nb; j += OKN_THREADS / 64) {
            const float v = okn_pose_row<T>(sW, joint ? b : 0.f, (const T*)a.tail + (size_t)(r0 + base + j) * a.ldt, D, lane);
            if (lane < OKN_MAXD) sA[j * OKN_MAXD + lane] = v;
        }
        __syncthreads();
        // ---- the state machine over the batch in window order, lane = joint
        if (wave == 0) {
            const int c = a.cls && lane < nb ? a.cls[r0 + base + lane] : 0;      // the class of row base + lane
            for (int j = 0; j < nb; ++j) {
                const int cj = __builtin_amdgcn_readlane(c, j);
                const size_t o = (size_t)(r0 + base + j) * OKN_MAXD + lane;
                if (joint) {
                    const float av = sA[j * OKN_MAXD + lane];
                    const float t = (av - lo) / span;
                    int q = rest;
                    if (t == t && cj >= 0) {                   // NaN, or the class "none": rest
                        const float f = fminf(fmaxf(t, 0.f), 1.f);
                        q = (int)rintf(f * (float)OKN_ONE);
                    }
                    if (len == V) sum -= sR[head * OKN_MAXD + lane];
                    sum += q;
                    sR[head * OKN_MAXD + lane] = q;
                    const int s = sum / (len == V ? V : len + 1);              // (both are >= 0: the floor)
                    out = s > out ? min(out + rate, s) : max(out - rate, s);
                    const float lvl = (float)out / (float)OKN_ONE;
                    const float scaled = lvl * span;
                    a.raw[o] = av;
                    a.pose[o] = out;
                    a.angle[o] = lo + scaled;
                } else if (lane < OKN_MAXD) {                  // the columns from D on: zero
                    a.raw[o] = 0.f;
                    a.pose[o] = 0;
                    a.angle[o] = 0.f;
                }
                if (len < V) ++len;
                head = head + 1 == V ? 0 : head + 1;
            }
        }
        __syncthreads();                                       // (sA is written again by the next batch; the ring is final)
    }

    for (int e = tid; e < OKN_MAXSMOOTH * OKN_MAXD / 4; e += OKN_THREADS) ((int4*)st->ring)[e] = ((const int4*)sR)[e];
    if (wave == 0) {
        if (joint) {
            st->out[lane] = out;
            st->sum[lane] = sum;
        }
        if (lane == 0) {
            st->head = head;
            st->len = len;
        }
    }
}

struct OknModelArgs {                    // what the host hands cp_online_kin_set_model's kernel
    int D;
    float lo[OKN_MAXD], span[OKN_MAXD];
    int rest[OKN_MAXD];
};

// the stream part of a state to its start: ring empty, out = 0
__device__ __forceinline__ void okn_restart(OknState* st, int tid) {
    for (int i = tid; i < OKN_MAXSMOOTH * OKN_MAXD; i += OKN_THREADS) st->ring[i] = 0;
    if (tid < OKN_MAXD) {
        st->out[tid] = 0;
        st->sum[tid] = 0;
    }
    if (tid == 0) {
        st->head = 0;
        st->len = 0;
    }
}

// installs a model from device memory (W [D][512], b [D]) and the host's lo, span and rest; rows from D on are zeroed and the
// stream restarts
__global__ __launch_bounds__(OKN_THREADS) void okn_set_model_kernel(OknState* st, const float* __restrict__ W, const float* __restrict__ b,
                                                                    OknModelArgs p) {
    const int tid = threadIdx.x;
    for (int e = tid; e < OKN_MAXD * OKN_F; e += OKN_THREADS) st->W[e] = e < p.D * OKN_F ? W[e] : 0.f;
    if (tid < OKN_MAXD) {
        const bool on = tid < p.D;
        st->b[tid] = on ? b[tid] : 0.f;
        st->lo[tid] = on ? p.lo[tid] : 0.f;
        st->span[tid] = on ? p.span[tid] : 0.f;
        st->rest[tid] = on ? p.rest[tid] : 0;
    }
    if (tid == 0) st->D = p.D;
    okn_restart(st, tid);
}

// the stream part of streams first .. first + gridDim.x - 1 to its start; the model stays
__global__ __launch_bounds__(OKN_THREADS) void okn_reset_kernel(OknState* states, int first) { okn_restart(states + first + blockIdx.x, threadIdx.x); }
