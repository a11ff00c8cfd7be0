// Closed-form head fit (include/cpnative.h, cp_online_readout_*): a user's projection (16 x 512 + 16) by ridge regression of the
// tail inputs u (cp_online_*tail_inputs) onto the unit class rows, without a gradient.  x = [u, 1] (513 values); per group
// (repetition) r the weighted moments G_r = sum w x x^T and C_r = sum w x E^[y]^T in float64; per plan (group mask, ridge) the
// normal equations (sum G_r + ridge D) X = sum C_r by Cholesky, and W = X[0..511]^T, b = X[512] in f32.  fit_reference and
// apply_reference of contrastiveprosthetics_amd/readout.py are the definitions; moments and solve equal them in every bit, and
// the apply is the push's tail by construction (ol_tile).
//
//   olr_index_kernel    grid n_groups, one wave per group: the windows of the group (0 <= slot < K, group == r) in window
//                       order, 64 at a time, placed by a ballot and a prefix count.
//   olr_moments_kernel  grid (45 tiles, n_groups).  The extended row x~ = [u (512), 1, E^[y] (16)] has 529 entries; the lower
//                       triangle of sum w x~ x~^T in 64 x 64 tiles holds G (rows and columns < 513) and C (rows 513..528,
//                       columns < 513).  A workgroup walks its group's index list in order, OLR_STAGE windows at a time staged
//                       in LDS as f32 (bf16 widened: exact) with their weights; thread (ty, tx) keeps a 4 x 4 register tile.
//                       Per window and element: p = (double)x_a * (double)x_b (exact), q = w * p, acc = acc + q, each
//                       rounded on its own.  The order of an element's sum is the window order: no slabs, no atomics.
//                       The f64 matrix instruction is not used: the order of its four-term inner sum is not documented, and
//                       the definition fixes one multiply by w and one add per window, which a fused dot product cannot give.
//   olr_solve_kernel    grid n_plans, OLR_SOLVE_THREADS threads, thread i owns row i.  The plan's matrix lives in scratch as
//                       M[j][i], i >= j (a column of L is contiguous across threads).  Cholesky by panels of OLR_NB columns:
//                       the panel's rows L[j0 + c][0..j0) are staged in LDS, every row i >= j0 subtracts k = 0..j0-1 in
//                       ascending k from its OLR_NB elements in registers (one read of L[i][k] serves the panel), then the
//                       panel's columns are finished one by one, k = j0.. ascending: element (i, j) sees its subtractions in
//                       k = 0..j-1 order, one rounded multiply and one rounded subtract each, as the definition has them.
//                       Forward substitution is column-oriented (row a takes k ascending as the y[k] become final), backward
//                       substitution follows the definition's order, k = a+1.. ascending, which only starts once x[a+1] is
//                       known: one lane per right-hand side walks row a of L, staged in LDS by all threads.
//   olr_round_kernel    W (P, 16, 512) f32 -> the compute dtype, as cp_online_*set_projection rounds it.
//   olr_apply_kernel    grid (chunks of OLR_APPLY_ROWS rows, P): ol_load_weights / ol_tile per 16-row tile, then z + b and
//                       z / sqrtf(ss) as ol_tail_tile forms them.
// Every value read from the device is checked before it is an index: a slot against K, a group against the grid, an index
// list's length and entries against n_rows.
#pragma once
#include "online_finetune.cuh"

constexpr int OLR_F = 512;                       // tail inputs per window
constexpr int OLR_X = OLR_F + 1;                 // x = [u, 1]
constexpr int OLR_E = OLR_X + CP_D_E;            // x~ = [u, 1, E^[y]]: 529
constexpr int OLR_TILE = 64;                     // a workgroup's tile of the moment matrix
constexpr int OLR_NT = (OLR_E + OLR_TILE - 1) / OLR_TILE;          // 9 tile rows
constexpr int OLR_TILES = OLR_NT * (OLR_NT + 1) / 2;              // 45 tiles of the lower triangle
constexpr int OLR_STAGE = 16;                    // windows staged in LDS at a time (the staging depth)
constexpr int OLR_MOM_THREADS = 256;
constexpr int OLR_MAXK = 64;                     // class slots (CP_ONLINE_MAX_CLASSES)
constexpr int OLR_MAX_GROUPS = 16;               // CP_ONLINE_READOUT_MAX_GROUPS
constexpr int OLR_MAX_PLANS = 256;               // CP_ONLINE_READOUT_MAX_PLANS
constexpr int OLR_LD = 520;                      // doubles per column of a plan's matrix and per right-hand side
constexpr int OLR_NB = 8;                        // columns per Cholesky panel
constexpr int OLR_SOLVE_THREADS = 576;           // nine waves: one thread per row, 513 of them in use
constexpr int OLR_PLAN_DOUBLES = OLR_X * OLR_LD;                  // a plan's matrix M: 513 columns (the right-hand sides live in LDS)
constexpr int OLR_SOLVE_LDS = (OLR_NB * OLR_LD + OLR_LD + OLR_LD * CP_D_E + 2 * CP_D_E) * 8;   // dynamic LDS of olr_solve_kernel
constexpr int OLR_APPLY_ROWS = 64;               // rows per workgroup of olr_apply_kernel
static_assert(OLR_X <= OLR_LD && OLR_X <= OLR_SOLVE_THREADS && OLR_MOM_THREADS == (OLR_TILE / 4) * (OLR_TILE / 4) && CP_D_E == 16,
              "readout layout");

// grid n_groups, 64 threads: idx[r][0..count[r]) = the windows w with 0 <= slot[w] < K and group[w] == r, ascending
__global__ __launch_bounds__(64) void olr_index_kernel(const int32_t* __restrict__ slot, const int32_t* __restrict__ group, int n_rows, int K,
                                                       int32_t* __restrict__ idx, int32_t* __restrict__ count) {
    const int lane = threadIdx.x, r = blockIdx.x;
    int32_t* out = idx + (size_t)r * n_rows;
    int n = 0;
    for (int base = 0; base < n_rows; base += 64) {
        const int w = base + lane;
        bool mine = false;
        if (w < n_rows) {
            const int s = slot[w];
            mine = s >= 0 && s < K && group[w] == r;
        }
        const unsigned long long m = __ballot(mine);
        if (mine) out[n + __popcll(m & ((1ull << lane) - 1ull))] = w;
        n += __popcll(m);
    }
    if (lane == 0) count[r] = n;
}

template <typename T>
struct OlrMomentsArgs {
    const T* u;                          // [n_rows][512]
    const int32_t* slot;                 // [n_rows]
    const double* weight;                // [n_rows]
    const float* targets;                // [K][16] unit class rows
    const int32_t* idx;                  // [n_groups][n_rows]
    const int32_t* count;                // [n_groups]
    double* G;                           // [n_groups][513][513], symmetric
    double* C;                           // [n_groups][513][16]
    int n_rows, K;
};

// entry a of x~ of window w with slot y (both checked by the caller)
template <typename T>
__device__ __forceinline__ float olr_entry(const OlrMomentsArgs<T>& a, int w, int y, int e) {
    if (e < OLR_F) return olf_widen<T>(a.u[(size_t)w * OLR_F + e]);
    if (e == OLR_F) return 1.f;
    if (e < OLR_E) return a.targets[y * CP_D_E + (e - OLR_X)];
    return 0.f;
}

template <typename T>
__global__ __launch_bounds__(OLR_MOM_THREADS) void olr_moments_kernel(OlrMomentsArgs<T> a) {
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
                    const int y = a.slot[w];
                    if (y >= 0 && y < a.K) {
                        v = olr_entry<T>(a, w, y, q < OLR_TILE ? a0 + q : b0 + q - OLR_TILE);
                        om = a.weight[w];
                    }
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
    double* C = a.C + (size_t)r * OLR_X * CP_D_E;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ea = a0 + ty * 4 + i, eb = b0 + tx * 4 + j;
            if (eb > ea || eb >= OLR_X || ea >= OLR_E) continue;
            if (ea < OLR_X) {
                G[(size_t)ea * OLR_X + eb] = acc[i][j];
                G[(size_t)eb * OLR_X + ea] = acc[i][j];
            } else {
                C[(size_t)eb * CP_D_E + (ea - OLR_X)] = acc[i][j];
            }
        }
}

struct OlrSolveArgs {
    const double* G;                     // [n_groups][513][513]
    const double* C;                     // [n_groups][513][16]
    double* scratch;                     // [n_plans][OLR_PLAN_DOUBLES]
    float* W;                            // [n_plans][16][512]
    float* b;                            // [n_plans][16]
    int32_t* status;                     // [n_plans]
    int n_groups;
    unsigned short mask[OLR_MAX_PLANS];
    double ridge[OLR_MAX_PLANS];
};

__global__ __launch_bounds__(OLR_SOLVE_THREADS) void olr_solve_kernel(OlrSolveArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double olr_smem[];      // OLR_SOLVE_LDS bytes (above the static 64 KB)
    double (*P)[OLR_LD] = (double (*)[OLR_LD])olr_smem;        // the panel's rows: P[c][k] = L[j0 + c][k], k < j0
    double* rowl = olr_smem + OLR_NB * OLR_LD;                 // backward substitution: row a of L
    double (*xs)[CP_D_E] = (double (*)[CP_D_E])(rowl + OLR_LD);            // [513][16]: the right-hand sides, then y, then x
    double (*ybuf)[CP_D_E] = (double (*)[CP_D_E])(rowl + OLR_LD + OLR_LD * CP_D_E);    // [2][16]
    const int tid = threadIdx.x, t = blockIdx.x, i = tid;
    const bool row = i < OLR_X;
    double* M = a.scratch + (size_t)t * OLR_PLAN_DOUBLES;      // M[j * OLR_LD + i], i >= j
    const unsigned mask = a.mask[t];
    const double lam = a.ridge[t];
    // ---- A = sum of G_r over the mask in ascending r, + ridge on the diagonal but for the bias; B likewise
    for (int j = 0; j < OLR_X; ++j) {
        if (row && i >= j) {
            double s = 0.0;
            for (int r = 0; r < a.n_groups; ++r)
                if ((mask >> r) & 1u) s = s + a.G[((size_t)r * OLR_X + j) * OLR_X + i];
            if (i == j && i < OLR_F) s = s + lam;
            M[(size_t)j * OLR_LD + i] = s;
        }
    }
    for (int e = tid; e < OLR_X * CP_D_E; e += OLR_SOLVE_THREADS) {
        double s = 0.0;
        for (int r = 0; r < a.n_groups; ++r)
            if ((mask >> r) & 1u) s = s + a.C[(size_t)r * OLR_X * CP_D_E + e];
        xs[e / CP_D_E][e % CP_D_E] = s;
    }
    __syncthreads();
    // ---- Cholesky, panel by panel
    int bad = 0;
    for (int j0 = 0; j0 < OLR_X && !bad; j0 += OLR_NB) {
        const int nb = min(OLR_NB, OLR_X - j0);
        for (int e = tid; e < OLR_NB * j0; e += OLR_SOLVE_THREADS) {
            const int c = e / j0, k = e % j0;
            P[c][k] = c < nb ? M[(size_t)k * OLR_LD + j0 + c] : 0.0;
        }
        __syncthreads();
        if (row && i >= j0) {
            double rr[OLR_NB];
#pragma unroll
            for (int c = 0; c < OLR_NB; ++c) rr[c] = c < nb && i >= j0 + c ? M[(size_t)(j0 + c) * OLR_LD + i] : 0.0;
            for (int k = 0; k < j0; ++k) {
                const double l = M[(size_t)k * OLR_LD + i];
#pragma unroll
                for (int c = 0; c < OLR_NB; ++c) {
                    const double p = l * P[c][k];
                    rr[c] = rr[c] - p;
                }
            }
#pragma unroll
            for (int c = 0; c < OLR_NB; ++c)
                if (c < nb && i >= j0 + c) M[(size_t)(j0 + c) * OLR_LD + i] = rr[c];
        }
        __syncthreads();
        for (int c = 0; c < nb; ++c) {
            const int j = j0 + c;
            const double piv = M[(size_t)j * OLR_LD + j];      // every thread reads the same values: the branch is uniform
            if (!(piv > 0.0) || !isfinite(piv)) {
                bad = j + 1;
                break;
            }
            const double ljj = sqrt(piv);
            double q[OLR_NB];
#pragma unroll
            for (int c2 = 0; c2 < OLR_NB; ++c2) q[c2] = c2 > c && c2 < nb ? M[(size_t)j * OLR_LD + j0 + c2] / ljj : 0.0;
            __syncthreads();                                   // column j has been read as the trailing update left it
            if (row && i == j) M[(size_t)j * OLR_LD + j] = ljj;
            if (row && i > j) {
                const double v = M[(size_t)j * OLR_LD + i] / ljj;
                M[(size_t)j * OLR_LD + i] = v;
#pragma unroll
                for (int c2 = 0; c2 < OLR_NB; ++c2)
                    if (c2 > c && c2 < nb && i >= j0 + c2) {
                        const double p = v * q[c2];
                        M[(size_t)(j0 + c2) * OLR_LD + i] = M[(size_t)(j0 + c2) * OLR_LD + i] - p;
                    }
            }
            __syncthreads();
        }
    }
    if (bad) {                                                 // (uniform)
        for (int e = tid; e < CP_D_E * OLR_F; e += OLR_SOLVE_THREADS) a.W[(size_t)t * CP_D_E * OLR_F + e] = 0.f;
        if (tid < CP_D_E) a.b[t * CP_D_E + tid] = 0.f;
        if (tid == 0) a.status[t] = bad;
        return;
    }
    // ---- forward substitution L y = B: y[k] = r[k] / L[k][k] becomes final, then every row a > k subtracts L[a][k] * y[k]
    double rr[CP_D_E];
#pragma unroll
    for (int d = 0; d < CP_D_E; ++d) rr[d] = row ? xs[i][d] : 0.0;
    for (int k = 0; k < OLR_X; ++k) {
        if (i == k) {
            const double lkk = M[(size_t)k * OLR_LD + k];
#pragma unroll
            for (int d = 0; d < CP_D_E; ++d) {
                rr[d] = rr[d] / lkk;
                ybuf[k & 1][d] = rr[d];
                xs[k][d] = rr[d];
            }
        }
        __syncthreads();                                       // (ybuf[k & 1] is written again at k + 2, behind the barrier of k + 1)
        if (row && i > k) {
            const double l = M[(size_t)k * OLR_LD + i];
#pragma unroll
            for (int d = 0; d < CP_D_E; ++d) {
                const double p = l * ybuf[k & 1][d];
                rr[d] = rr[d] - p;
            }
        }
    }
    __syncthreads();
    // ---- backward substitution L^T x = y: x[a] = (y[a] - sum over k = a+1..512 ascending of L[k][a] * x[k]) / L[a][a]
    for (int aa = OLR_X - 1; aa >= 0; --aa) {
        if (row && i >= aa) rowl[i] = M[(size_t)aa * OLR_LD + i];
        __syncthreads();
        if (tid < CP_D_E) {
            double s = xs[aa][tid];
            for (int k = aa + 1; k < OLR_X; ++k) {
                const double p = rowl[k] * xs[k][tid];
                s = s - p;
            }
            xs[aa][tid] = s / rowl[aa];
        }
        __syncthreads();
    }
    for (int e = tid; e < CP_D_E * OLR_F; e += OLR_SOLVE_THREADS) a.W[(size_t)t * CP_D_E * OLR_F + e] = (float)xs[e % OLR_F][e / OLR_F];
    if (tid < CP_D_E) a.b[t * CP_D_E + tid] = (float)xs[OLR_F][tid];
    if (tid == 0) a.status[t] = 0;
}

// W (n, f32) -> the compute dtype, as olf_set_projection_kernel rounds it
template <typename T>
__global__ __launch_bounds__(256) void olr_round_kernel(const float* __restrict__ W, T* __restrict__ Wd, long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) Wd[e] = ol_cvt<T>(W[e]);
}

struct OlrApplyArgs {
    const void* u;                       // [n_rows][512] in T
    const void* wT;                      // [n_plans][16][512] in T
    const float* b;                      // [n_plans][16]
    float* out;                          // [n_plans][n_rows][16]
    int n_rows;
};

// grid (chunks of OLR_APPLY_ROWS rows, n_plans)
template <typename T>
__global__ __launch_bounds__(OL_THREADS) void olr_apply_kernel(OlrApplyArgs a) {
#pragma clang fp contract(off)
    __shared__ OlTileLds<T> L;
    const int tid = threadIdx.x, p = blockIdx.y;
    OlLayerArgs proj{};
    proj.act = a.u;
    proj.w = (const T*)a.wT + (size_t)p * CP_D_E * OLR_F;
    proj.bias = a.b + p * CP_D_E;
    proj.K = OLR_F;
    proj.F = CP_D_E;
    uint4 wf[OL_MAXCH][OL_KC * (int)sizeof(T) / 64];
    ol_load_weights<T>((const T*)proj.w, OLR_F, 0, wf);
    const int row_begin = blockIdx.x * OLR_APPLY_ROWS, row_end = min(a.n_rows, row_begin + OLR_APPLY_ROWS);
    float* out = a.out + (size_t)p * a.n_rows * CP_D_E;
    for (int m0 = row_begin; m0 < row_end; m0 += 16) {
        ol_tile<T, false>(proj, L, OLR_F, 0, m0, a.n_rows, wf);
        if (tid < 16 && m0 + tid < row_end) {                  // as ol_tail_tile: z, then z / sqrtf(ss), in f32
            float z[16], ss = 0.f;
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                z[d] = L.red[0][tid][d] + proj.bias[d];
                ss += z[d] * z[d];
            }
            const float nrm = sqrtf(ss);
#pragma unroll
            for (int d = 0; d < 16; ++d) out[(size_t)(m0 + tid) * 16 + d] = z[d] / nrm;
        }
        // the next tile's staging writes only L.a; red[0] is rewritten behind ol_tile's first barrier
    }
}
