// Pose filter (include/cpnative.h, cp_online_kf_*): a steady-state Kalman stage behind the joint readout.  The state is
// x = [theta (D), omega (D)] around the resting pose c; a trajectory model A, W is fitted to the glove, a measurement noise Q to
// the readout's held-out error, the Riccati recursion is iterated to a fixed gain, and the stage then runs x' = M x + K o per
// window.  The numpy definitions are in contrastiveprosthetics_amd/kalman.py (moments_reference, design_reference,
// FilterReference, sweep_reference); every kernel here equals them in every bit, float64 words included.
//
//   okf_moments_kernel   grid n_groups, one workgroup per group.  The windows are walked in order, OKF_STAGE at a time: the rows
//                        [s_k, s_{k+1}, e_{k+1}] (5 D f32 values) of the counted k are built on the device and staged in LDS, and
//                        the 3 (2D)^2 + D^2 entries of G, C, S and E are spread over the threads, each with its own f64 register:
//                        per counted k one exact product and one rounded add, in window order.  No slabs, no atomics.
//   okf_design_kernel    grid n_plans (at most OKF_PLANS_PER_LAUNCH a launch), one workgroup per plan.  Four (2D) x (2D + 1) f64
//                        matrices, K^T and the innovation matrix live in LDS (at most 158,208 bytes); W and Q of the plan in
//                        scratch.  Every inner product runs with its index ascending from +0.0, one rounded multiply and one
//                        rounded add each; Cholesky element (i, j) takes its subtractions in k = 0..j-1 order; the forward
//                        substitution takes k ascending and the backward one k descending, as the definition has them.
//   okf_step             the filter step of one row on one wave (device function; the sweep and the stage both call it): lane i
//                        holds x_i and the rows M[i], K[i] in registers; x_j and o_j come by v_readlane.
//   okf_sweep_kernel     grid n_plans, one wave per plan: the filter over the plan's held-out windows in window order, restarted at
//                        every run, and the eight f64 sums per joint; optionally the filtered sequence.
//   okf_push_kernel      grid n_streams, four waves per stream, one launch per push.  The readout W (at most 64 KB), M (16 KB) and
//                        K (8 KB) are staged in LDS once; the four waves share the rows of a batch for the matvec (okn_pose_row,
//                        unchanged), then wave 0 runs the filter step and the integer tail over the batch in window order.  A
//                        stream without rows, without a model or with rows outside the launch is left untouched.
//   okf_set_model_kernel, okf_reset_kernel   one workgroup per stream.
// Everything is integer or single f32 / f64 operations with floating-point contraction off and plain vector stores: no
// floating-point atomics, no grid-wide barrier, no persistent kernel.
#pragma once
#include "online_kinematics.cuh"

constexpr int OKF_MAXD = OKN_MAXD;               // joints
constexpr int OKF_MAXS = 2 * OKF_MAXD;           // state components
constexpr int OKF_THREADS = 256;
constexpr int OKF_STAGE = 16;                    // windows staged in LDS at a time (moments)
constexpr int OKF_ROW = 5 * OKF_MAXD;            // [s_k, s_{k+1}, e_{k+1}]
constexpr int OKF_MOM_ENTRIES = (3 * OKF_MAXS * OKF_MAXS + OKF_MAXD * OKF_MAXD + OKF_THREADS - 1) / OKF_THREADS;   // 52 per thread
constexpr int OKF_PLANS_PER_LAUNCH = 128;        // (a plan's settings travel in the kernel arguments)
constexpr int OKF_MAX_ITERS = 1024;              // CP_ONLINE_KF_MAX_ITERS
constexpr int OKF_SUMS = 8;                      // okn's seven and the jitter sum
constexpr int OKF_PLAN_DOUBLES = OKF_MAXS * OKF_MAXS + OKF_MAXD * OKF_MAXD;            // a plan's W and Q in scratch
constexpr int OKF_PUSH_LDS = OKN_APPLY_LDS + OKN_BATCH * OKN_MAXD * 4 + OKF_MAXS * OKF_MAXS * 4 + OKF_MAXS * OKF_MAXD * 4;
__host__ __device__ constexpr int okf_design_doubles(int D) { return 4 * (2 * D) * (2 * D + 1) + D * (2 * D + 1) + D * (D + 1); }
constexpr int OKF_DESIGN_LDS = okf_design_doubles(OKF_MAXD) * 8;
static_assert(OKF_DESIGN_LDS <= 160 * 1024 && OKF_PUSH_LDS <= 160 * 1024, "the design and the stage fit the CU's LDS");

// ---------------------------------------------------------------------------------------
// moments
// ---------------------------------------------------------------------------------------
struct OkfMomentsArgs {
    const float* a;                      // [n_rows][D] the readout's prediction
    const float* y;                      // [n_rows][D] targets
    const int32_t* group;                // [n_rows]
    double* G;                           // [n_groups][2D][2D]
    double* C;                           // [n_groups][2D][2D]
    double* S;                           // [n_groups][2D][2D]
    double* E;                           // [n_groups][D][D]
    int32_t* count;                      // [n_groups]
    int n_rows, D;
    float c[OKF_MAXD];                   // the centre
};

__global__ __launch_bounds__(OKF_THREADS) void okf_moments_kernel(OkfMomentsArgs a) {
#pragma clang fp contract(off)
    __shared__ float rows[OKF_STAGE][OKF_ROW];
    __shared__ int flag[OKF_STAGE];
    const int tid = threadIdx.x, r = blockIdx.x, D = a.D, n2 = 2 * D, nn = n2 * n2, row = 5 * D, total = 3 * nn + D * D;
    int off[OKF_MOM_ENTRIES];                                  // entry tid + 256 i: its two positions in the row, or -1
    double acc[OKF_MOM_ENTRIES];
#pragma unroll
    for (int i = 0; i < OKF_MOM_ENTRIES; ++i) {
        const int e = tid + OKF_THREADS * i;
        acc[i] = 0.0;
        off[i] = -1;
        if (e < 3 * nn) {
            const int blk = e / nn, rem = e % nn, p = rem / n2, q = rem % n2;
            off[i] = ((blk >= 1 ? n2 : 0) + p) | (((blk == 2 ? n2 : 0) + q) << 16);     // G: s_k s_k, C: s_{k+1} s_k, S: s_{k+1} s_{k+1}
        } else if (e < total) {
            const int rem = e - 3 * nn;
            off[i] = (2 * n2 + rem / D) | ((2 * n2 + rem % D) << 16);
        }
    }
    int n = 0;
    for (int base = 1; base + 1 < a.n_rows; base += OKF_STAGE) {
        __syncthreads();                                       // the stage before has been read
        for (int e = tid; e < OKF_STAGE * row; e += OKF_THREADS) {
            const int s = e / row, q = e % row, k = base + s;
            const bool on = k + 1 < a.n_rows && a.group[k - 1] == r && a.group[k] == r && a.group[k + 1] == r;
            float v = 0.f;
            if (on) {
                const int part = q / D, d = q % D;
                const float cd = a.c[d];
                const float* y0 = a.y + (size_t)k * D + d;     // y_k[d]; y0[-D] and y0[D] are its neighbours
                if (part == 0) v = y0[0] - cd;
                else if (part == 1) {
                    const float t1 = y0[0] - cd, t0 = y0[-D] - cd;
                    v = t1 - t0;
                } else if (part == 2) v = y0[D] - cd;
                else if (part == 3) {
                    const float t2 = y0[D] - cd, t1 = y0[0] - cd;
                    v = t2 - t1;
                } else v = a.a[(size_t)(k + 1) * D + d] - y0[D];
            }
            rows[s][q] = v;
            if (q == 0) flag[s] = on ? 1 : 0;
        }
        __syncthreads();
        for (int s = 0; s < OKF_STAGE; ++s) {
            if (!flag[s]) continue;                            // (uniform)
            ++n;
#pragma unroll
            for (int i = 0; i < OKF_MOM_ENTRIES; ++i)
                if (off[i] >= 0) {
                    const double p = (double)rows[s][off[i] & 0xffff] * (double)rows[s][off[i] >> 16];    // exact: two f32 values
                    acc[i] = acc[i] + p;
                }
        }
    }
#pragma unroll
    for (int i = 0; i < OKF_MOM_ENTRIES; ++i) {
        const int e = tid + OKF_THREADS * i;
        if (e < nn) a.G[(size_t)r * nn + e] = acc[i];
        else if (e < 2 * nn) a.C[(size_t)r * nn + e - nn] = acc[i];
        else if (e < 3 * nn) a.S[(size_t)r * nn + e - 2 * nn] = acc[i];
        else if (e < total) a.E[(size_t)r * D * D + e - 3 * nn] = acc[i];
    }
    if (tid == 0) a.count[r] = n;
}

// ---------------------------------------------------------------------------------------
// design
// ---------------------------------------------------------------------------------------
struct OkfDesignArgs {
    const double* G;                     // [n_groups][2D][2D]
    const double* C;
    const double* S;
    const double* E;                     // [n_groups][D][D]
    const int32_t* count;                // [n_groups]
    double* scratch;                     // [plans of this launch][OKF_PLAN_DOUBLES]
    float* M;                            // [plans][2D][2D]
    float* K;                            // [plans][2D][D]
    double* delta;                       // [plans]
    int32_t* status;                     // [plans]
    int D, n_groups;
    unsigned short mask[OKF_PLANS_PER_LAUNCH], iters[OKF_PLANS_PER_LAUNCH];
    double lam[OKF_PLANS_PER_LAUNCH], rho[OKF_PLANS_PER_LAUNCH], kappa[OKF_PLANS_PER_LAUNCH];
};

// Cholesky of the n x n matrix in the lower triangle of Mx (leading dimension ld), in place; false at the first pivot that is
// not positive (uniform over the workgroup).  Element (i, j) takes its subtractions in k = 0..j-1 order.
__device__ __forceinline__ bool okf_chol(double* Mx, int n, int ld, double* piv_sh, int tid) {
#pragma clang fp contract(off)
    for (int j = 0; j < n; ++j) {
        double s = 0.0;
        if (tid >= j && tid < n) {
            s = Mx[tid * ld + j];
            for (int k = 0; k < j; ++k) {
                const double p = Mx[tid * ld + k] * Mx[j * ld + k];
                s = s - p;
            }
        }
        if (tid == j) piv_sh[0] = s;
        __syncthreads();
        const double piv = piv_sh[0];
        if (!(piv > 0.0)) return false;
        const double ljj = sqrt(piv);
        if (tid == j) Mx[j * ld + j] = ljj;
        else if (tid > j && tid < n) Mx[tid * ld + j] = s / ljj;
        __syncthreads();
    }
    return true;
}

// L L^T X = B in place, B n x m (leading dimension ldb), one thread per column: forward with k ascending, backward with k
// descending
__device__ __forceinline__ void okf_solve(const double* L, int n, int ld, double* B, int m, int ldb, int tid) {
#pragma clang fp contract(off)
    if (tid < m) {
        for (int a = 0; a < n; ++a) {
            double s = B[a * ldb + tid];
            for (int k = 0; k < a; ++k) {
                const double p = L[a * ld + k] * B[k * ldb + tid];
                s = s - p;
            }
            B[a * ldb + tid] = s / L[a * ld + a];
        }
        for (int a = n - 1; a >= 0; --a) {
            double s = B[a * ldb + tid];
            for (int k = n - 1; k > a; --k) {
                const double p = L[k * ld + a] * B[k * ldb + tid];
                s = s - p;
            }
            B[a * ldb + tid] = s / L[a * ld + a];
        }
    }
    __syncthreads();
}

// J = I - K H, K^T in Z (D x 2D, leading dimension LD)
__device__ __forceinline__ double okf_J(const double* Z, int LD, int D, int i, int k) {
#pragma clang fp contract(off)
    const double e = i == k ? 1.0 : 0.0;
    return k < D ? e - Z[k * LD + i] : e;
}

__global__ __launch_bounds__(OKF_THREADS) void okf_design_kernel(OkfDesignArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double okf_dsmem[];
    const int tid = threadIdx.x, t = blockIdx.x, D = a.D, n2 = 2 * D, LD = n2 + 1, nn = n2 * n2, dd = D * D, LS = D + 1, R = a.n_groups;
    double* m0 = okf_dsmem;
    double* m1 = m0 + n2 * LD;
    double* m2 = m1 + n2 * LD;
    double* m3 = m2 + n2 * LD;
    double* Z = m3 + n2 * LD;                                  // [D][LD]: K^T
    double* Ls = Z + D * LD;                                   // [D][D + 1]: the innovation matrix and its factor
    __shared__ double piv_sh[1];
    __shared__ double red[2][OKF_THREADS];
    double* Wg = a.scratch + (size_t)t * OKF_PLAN_DOUBLES;
    double* Qg = Wg + OKF_MAXS * OKF_MAXS;
    float* Mo = a.M + (size_t)t * nn;
    float* Ko = a.K + (size_t)t * n2 * D;
    const unsigned mask = a.mask[t];
    const int T = a.iters[t];
    const double lam = a.lam[t], rho = a.rho[t], kappa = a.kappa[t];

    long long n = 0;
    for (int r = 0; r < R; ++r)
        if ((mask >> r) & 1u) n += a.count[r] > 0 ? a.count[r] : 0;
    const double nd = (double)n;
    auto fail = [&](int code) {                                // (uniform)
        for (int e = tid; e < nn; e += OKF_THREADS) Mo[e] = 0.f;
        for (int e = tid; e < n2 * D; e += OKF_THREADS) Ko[e] = 0.f;
        if (tid == 0) {
            a.delta[t] = __longlong_as_double(0x7ff0000000000000ll);
            a.status[t] = code;
        }
    };
    if (n < n2 + 1) return fail(1);
    auto gsum = [&](const double* X, int sz, int e) {          // the groups of the mask in ascending order, from +0.0, then / n
        double s = 0.0;
        for (int r = 0; r < R; ++r)
            if ((mask >> r) & 1u) s = s + X[(size_t)r * sz + e];
        return s / nd;
    };

    // ---- A: (G + lambda I) A^T = C^T
    for (int e = tid; e < nn; e += OKF_THREADS) {
        const int i = e / n2, j = e % n2;
        m0[i * LD + j] = gsum(a.G, nn, e);
        m1[i * LD + j] = gsum(a.C, nn, j * n2 + i);
    }
    __syncthreads();
    {
        double tr = 0.0;
        for (int i = 0; i < n2; ++i) tr = tr + m0[i * LD + i];
        const double lt = lam * tr;
        const double lamv = lt / (double)n2;
        __syncthreads();
        if (tid < n2) m0[tid * LD + tid] = m0[tid * LD + tid] + lamv;
        __syncthreads();
    }
    if (!okf_chol(m0, n2, LD, piv_sh, tid)) return fail(2);
    okf_solve(m0, n2, LD, m1, n2, LD, tid);
    for (int e = tid; e < nn; e += OKF_THREADS) {
        const int i = e / n2, j = e % n2;
        m2[i * LD + j] = m1[j * LD + i];                       // A
    }
    __syncthreads();
    // ---- W = rho (sym(S - A C^T - C A^T + A G A^T) + w0 I)
    for (int e = tid; e < nn; e += OKF_THREADS) {
        const int i = e / n2, j = e % n2;
        m0[i * LD + j] = gsum(a.G, nn, e);
        m1[i * LD + j] = gsum(a.C, nn, e);
    }
    __syncthreads();
    for (int e = tid; e < nn; e += OKF_THREADS) {
        const int i = e / n2, j = e % n2;
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < n2; ++k) {
            const double p1 = m2[i * LD + k] * m1[j * LD + k];             // A C^T
            s1 = s1 + p1;
            const double p2 = m2[i * LD + k] * m0[k * LD + j];             // A G
            s2 = s2 + p2;
        }
        m3[i * LD + j] = s1;
        Wg[e] = s2;                                           // A G, parked in scratch until m1 is free
    }
    __syncthreads();
    for (int e = tid; e < nn; e += OKF_THREADS) m1[(e / n2) * LD + e % n2] = Wg[e];    // A G
    __syncthreads();
    for (int e = tid; e < nn; e += OKF_THREADS) {
        const int i = e / n2, j = e % n2;
        double s = 0.0;
        for (int k = 0; k < n2; ++k) {
            const double p = m1[i * LD + k] * m2[j * LD + k];              // (A G) A^T
            s = s + p;
        }
        const double r1 = gsum(a.S, nn, e) - m3[i * LD + j];
        const double r2 = r1 - m3[j * LD + i];
        m0[i * LD + j] = r2 + s;
    }
    __syncthreads();
    {
        double trS = 0.0, trE = 0.0;
        for (int i = 0; i < n2; ++i) trS = trS + gsum(a.S, nn, i * n2 + i);
        for (int i = 0; i < D; ++i) trE = trE + gsum(a.E, dd, i * D + i);
        const double w1 = 1e-6 * trS, q1 = 1e-6 * trE;
        const double w0 = w1 / (double)n2, q0 = q1 / (double)D;
        for (int e = tid; e < nn; e += OKF_THREADS) {
            const int i = e / n2, j = e % n2;
            const double sum = m0[i * LD + j] + m0[j * LD + i];
            double v = 0.5 * sum;
            if (i == j) v = v + w0;
            v = rho * v;
            Wg[e] = v;
            m1[i * LD + j] = v;                                // P_0 = W
        }
        for (int e = tid; e < dd; e += OKF_THREADS) {
            double v = gsum(a.E, dd, e);
            if (e / D == e % D) v = v + q0;
            Qg[e] = kappa * v;
        }
    }
    __syncthreads();

    // ---- the Riccati recursion: P in m1, A in m2
    double dmax = 0.0, pmax = 0.0;
    for (int it = 0; it < T; ++it) {
        for (int e = tid; e < nn; e += OKF_THREADS) {          // A P
            const int i = e / n2, j = e % n2;
            double s = 0.0;
            for (int k = 0; k < n2; ++k) {
                const double p = m2[i * LD + k] * m1[k * LD + j];
                s = s + p;
            }
            m0[i * LD + j] = s;
        }
        __syncthreads();
        for (int e = tid; e < nn; e += OKF_THREADS) {          // P- = A P A^T + W, the lower triangle
            const int i = e / n2, j = e % n2;
            if (j > i) continue;
            double s = 0.0;
            for (int k = 0; k < n2; ++k) {
                const double p = m0[i * LD + k] * m2[j * LD + k];
                s = s + p;
            }
            m3[i * LD + j] = s + Wg[e];
        }
        __syncthreads();
        for (int e = tid; e < nn; e += OKF_THREADS) {
            const int i = e / n2, j = e % n2;
            if (j > i) m3[i * LD + j] = m3[j * LD + i];
        }
        __syncthreads();
        for (int e = tid; e < dd; e += OKF_THREADS) Ls[(e / D) * LS + e % D] = m3[(e / D) * LD + e % D] + Qg[e];
        for (int e = tid; e < D * n2; e += OKF_THREADS) Z[(e / n2) * LD + e % n2] = m3[(e / n2) * LD + e % n2];
        __syncthreads();
        if (!okf_chol(Ls, D, LS, piv_sh, tid)) return fail(3);
        okf_solve(Ls, D, LS, Z, n2, LD, tid);                  // Z = K^T
        for (int e = tid; e < nn; e += OKF_THREADS) {          // (I - K H) P-
            const int i = e / n2, j = e % n2;
            double s = 0.0;
            for (int k = 0; k < n2; ++k) {
                const double p = okf_J(Z, LD, D, i, k) * m3[k * LD + j];
                s = s + p;
            }
            m0[i * LD + j] = s;
        }
        __syncthreads();
        for (int e = tid; e < n2 * D; e += OKF_THREADS) {      // K Q (m3 is free: the P- above has been read)
            const int i = e / D, d = e % D;
            double s = 0.0;
            for (int q = 0; q < D; ++q) {
                const double p = Z[q * LD + i] * Qg[q * D + d];
                s = s + p;
            }
            m3[i * LD + d] = s;
        }
        __syncthreads();
        for (int e = tid; e < nn; e += OKF_THREADS) {          // P = (I - K H) P- (I - K H)^T + K Q K^T, the lower triangle
            const int i = e / n2, j = e % n2;
            if (j > i) continue;
            double s1 = 0.0, s2 = 0.0;
            for (int k = 0; k < n2; ++k) {
                const double p = m0[i * LD + k] * okf_J(Z, LD, D, j, k);
                s1 = s1 + p;
            }
            for (int d = 0; d < D; ++d) {
                const double p = m3[i * LD + d] * Z[d * LD + j];
                s2 = s2 + p;
            }
            const double v = s1 + s2;
            if (it == T - 1) {
                dmax = fmax(dmax, fabs(v - m1[i * LD + j]));
                pmax = fmax(pmax, fabs(v));
            }
            m1[i * LD + j] = v;
        }
        __syncthreads();
        for (int e = tid; e < nn; e += OKF_THREADS) {
            const int i = e / n2, j = e % n2;
            if (j > i) m1[i * LD + j] = m1[j * LD + i];
        }
        __syncthreads();
    }

    // ---- M = (I - K H) A and K in f32, delta
    for (int e = tid; e < nn; e += OKF_THREADS) {
        const int i = e / n2, j = e % n2;
        double s = 0.0;
        for (int k = 0; k < n2; ++k) {
            const double p = okf_J(Z, LD, D, i, k) * m2[k * LD + j];
            s = s + p;
        }
        Mo[e] = (float)s;
    }
    for (int e = tid; e < n2 * D; e += OKF_THREADS) Ko[e] = (float)Z[(e % D) * LD + e / D];
    red[0][tid] = dmax;
    red[1][tid] = pmax;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < OKF_THREADS; ++i) {
            dmax = fmax(dmax, red[0][i]);
            pmax = fmax(pmax, red[1][i]);
        }
        a.delta[t] = dmax / pmax;
        a.status[t] = 0;
    }
}

// ---------------------------------------------------------------------------------------
// the filter step
// ---------------------------------------------------------------------------------------
// One row on one wave, every lane of the wave in it.  Lane i < 2D holds x_i and the rows Mr = M[i][0..2D), Kr = K[i][0..D)
// (zeros elsewhere); a_lane and c_lane are the readout and the centre of joint `lane` on the lanes below D.  Returns
// filtered_lane = x_lane + c_lane (lanes below D), a quiet NaN while the stream has not started.
__device__ __forceinline__ float okf_step(const float (&Mr)[OKF_MAXS], const float (&Kr)[OKF_MAXD], float& x, int& started, float a_lane,
                                          float c_lane, int D, int lane) {
#pragma clang fp contract(off)
    const float o = lane < D ? a_lane - c_lane : 0.f;
    const bool fin = __ballot(lane < D && !(fabsf(o) <= 3.402823466e+38f)) == 0ull;    // every o finite
    if (!started) {
        if (fin) {
            x = lane < D ? o : 0.f;
            started = 1;
        }
    } else if (fin) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < OKF_MAXS; ++j)
            if (j < 2 * D) {
                const float xj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
                const float p = Mr[j] * xj;
                acc = acc + p;
            }
#pragma unroll
        for (int j = 0; j < OKF_MAXD; ++j)
            if (j < D) {
                const float oj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o), j));
                const float p = Kr[j] * oj;
                acc = acc + p;
            }
        x = acc;
    }
    return started ? x + c_lane : __int_as_float(0x7fc00000);
}

// ---------------------------------------------------------------------------------------
// held-out sweep
// ---------------------------------------------------------------------------------------
struct OkfSweepArgs {
    const float* a;                      // [n_rows][D]
    const float* y;                      // [n_rows][D]
    const int32_t* group;                // [n_rows]
    const float* M;                      // [n_plans][2D][2D]
    const float* K;                      // [n_plans][2D][D]
    double* sums;                        // [n_plans][D][8]
    float* filtered;                     // [n_plans][n_rows][D] or NULL
    int n_rows, D;
    float c[OKF_MAXD];
    unsigned short mask[OLR_MAX_PLANS];
};

__global__ __launch_bounds__(64) void okf_sweep_kernel(OkfSweepArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, p = blockIdx.x, D = a.D, n2 = 2 * D;
    const unsigned mask = a.mask[p];
    const bool joint = lane < D;
    float Mr[OKF_MAXS], Kr[OKF_MAXD];
#pragma unroll
    for (int j = 0; j < OKF_MAXS; ++j) Mr[j] = lane < n2 && j < n2 ? a.M[((size_t)p * n2 + lane) * n2 + j] : 0.f;
#pragma unroll
    for (int j = 0; j < OKF_MAXD; ++j) Kr[j] = lane < n2 && j < D ? a.K[((size_t)p * n2 + lane) * D + j] : 0.f;
    const float c = joint ? a.c[lane] : 0.f;
    const float nanv = __int_as_float(0x7fc00000);
    float* fout = a.filtered ? a.filtered + (size_t)p * a.n_rows * D : nullptr;
    double s[OKF_SUMS];
#pragma unroll
    for (int k = 0; k < OKF_SUMS; ++k) s[k] = 0.0;
    float x = 0.f, prev = 0.f;
    int started = 0, gprev = -1;
    bool have_prev = false;
    constexpr int U = 8;                                       // rows whose loads are in flight together
    for (int base = 0; base < a.n_rows; base += U) {
        int g[U];
        float av[U], yv[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = min(base + k, a.n_rows - 1);
            g[k] = a.group[i];
            av[k] = joint ? a.a[(size_t)i * D + lane] : 0.f;
            yv[k] = joint ? a.y[(size_t)i * D + lane] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (base + k >= a.n_rows) break;                   // (uniform)
            const int gk = g[k];
            const bool in = gk >= 0 && gk < OLR_MAX_GROUPS && ((mask >> gk) & 1u);
            const bool fresh = base + k == 0 || gprev != gk;   // the window before is not this group's: a run starts
            gprev = gk;
            if (!in) {
                if (fout && joint) fout[(size_t)(base + k) * D + lane] = nanv;
                continue;
            }
            if (fresh) {
                x = 0.f;
                started = 0;
                have_prev = false;
            }
            const float f = okf_step(Mr, Kr, x, started, av[k], c, D, lane);
            if (!joint) continue;
            if (fout) fout[(size_t)(base + k) * D + lane] = f;
            if (f == f) {
                const double y = (double)yv[k], q = (double)f;
                const double yy = y * y, qq = q * q, yq = y * q, e = q - y;
                const double ee = e * e;
                s[0] = s[0] + 1.0;
                s[1] = s[1] + y;
                s[2] = s[2] + yy;
                s[3] = s[3] + q;
                s[4] = s[4] + qq;
                s[5] = s[5] + yq;
                s[6] = s[6] + ee;
                if (have_prev) {
                    const double dq = q - (double)prev;
                    const double d2 = dq * dq;
                    s[7] = s[7] + d2;
                }
                prev = f;
                have_prev = true;
            } else have_prev = false;
        }
    }
    if (joint)
#pragma unroll
        for (int k = 0; k < OKF_SUMS; ++k) a.sums[((size_t)p * D + lane) * OKF_SUMS + k] = s[k];
}

// ---------------------------------------------------------------------------------------
// the stage
// ---------------------------------------------------------------------------------------
// Per-stream state.  A zeroed state is a valid start: no model, not started, pose 0.
struct OkfState {
    int D;                               // ---- model part (survives a reset); 0: no model
    int started;                         // ---- stream part
    int pad[6];
    float x[OKF_MAXS];                   // the state [theta, omega] around the centre
    int out[OKF_MAXD];                   // the pose, integers out of 4096
    int rest[OKF_MAXD];                  // ---- model
    float lo[OKF_MAXD], span[OKF_MAXD], b[OKF_MAXD], c[OKF_MAXD];
    float M[OKF_MAXS * OKF_MAXS];        // [i][64]
    float K[OKF_MAXS * OKF_MAXD];        // [i][32]
    float W[OKF_MAXD * OKN_F];           // [joint][512]
};

struct OkfPushArgs {
    OkfState* states;
    const void* tail;                    // [total_rows][ldt] in T
    const int32_t* cls;                  // [total_rows] class id or -1, or NULL
    const int32_t* row0;                 // [n_streams]
    const int32_t* m;                    // [n_streams]
    int ldt, total_rows, rate;
    float* raw;                          // [total_rows][32]
    float* filtered;                     // [total_rows][32]
    int32_t* pose;                       // [total_rows][32]
    float* angle;                        // [total_rows][32]
};

template <typename T>
__global__ __launch_bounds__(OKF_THREADS) void okf_push_kernel(OkfPushArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float okf_smem[];
    float* sW = okf_smem;                                      // [D][512]
    float* sA = sW + OKN_MAXD * OKN_F;                         // [OKN_BATCH][32]: a of the batch's rows
    float* sM = sA + OKN_BATCH * OKN_MAXD;                     // [64][64]
    float* sK = sM + OKF_MAXS * OKF_MAXS;                      // [64][32]
    OkfState* st = a.states + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, jl = lane & (OKF_MAXD - 1);
    const int D = st->D, Mrows = a.m[blockIdx.x], r0 = a.row0[blockIdx.x], rate = a.rate;
    // a stream without a model, or whose rows disagree with the limits, is left untouched (uniform over the workgroup)
    if (D < 1 || D > OKF_MAXD || Mrows < 1 || Mrows > OKN_MAXM || r0 < 0 || r0 > a.total_rows - Mrows || rate < 1 || rate > OKN_ONE ||
        a.ldt < OKN_F)
        return;
    {
        const float4* W4 = (const float4*)st->W;
        const float4* M4 = (const float4*)st->M;               // (M and K are contiguous in the state and in LDS)
        for (int e = tid; e < D * (OKN_F / 4); e += OKF_THREADS) ((float4*)sW)[e] = W4[e];
        for (int e = tid; e < (OKF_MAXS * OKF_MAXS + OKF_MAXS * OKF_MAXD) / 4; e += OKF_THREADS) ((float4*)sM)[e] = M4[e];
    }
    const bool joint = lane < D;
    const float b = st->b[jl], lo = st->lo[jl], span = st->span[jl], c = joint ? st->c[jl] : 0.f;
    const int rest = st->rest[jl];
    int out = st->out[jl], started = st->started != 0;
    float x = st->x[lane];
    __syncthreads();
    float Mr[OKF_MAXS], Kr[OKF_MAXD];
    if (wave == 0) {
#pragma unroll
        for (int j = 0; j < OKF_MAXS; ++j) Mr[j] = sM[lane * OKF_MAXS + j];
#pragma unroll
        for (int j = 0; j < OKF_MAXD; ++j) Kr[j] = sK[lane * OKF_MAXD + j];
    }

    for (int base = 0; base < Mrows; base += OKN_BATCH) {
        const int nb = min(OKN_BATCH, Mrows - base);
        for (int j = wave; j < nb; j += OKF_THREADS / 64) {    // the matvec: row j of the batch on wave j % 4
            const float v = okn_pose_row<T>(sW, joint ? b : 0.f, (const T*)a.tail + (size_t)(r0 + base + j) * a.ldt, D, lane);
            if (lane < OKF_MAXD) sA[j * OKF_MAXD + lane] = v;
        }
        __syncthreads();
        if (wave == 0) {                                       // the filter and the integer tail over the batch in window order
            const int cl = a.cls && lane < nb ? a.cls[r0 + base + lane] : 0;
            for (int j = 0; j < nb; ++j) {
                const int cj = __builtin_amdgcn_readlane(cl, j);
                const size_t o = (size_t)(r0 + base + j) * OKF_MAXD + lane;
                const float av = lane < OKF_MAXD ? sA[j * OKF_MAXD + lane] : 0.f;
                const float f = okf_step(Mr, Kr, x, started, av, c, D, lane);
                if (joint) {
                    const float t = (f - lo) / span;
                    int q = rest;
                    if (t == t && cj >= 0) {                   // NaN, or the class "none": rest
                        const float u = fminf(fmaxf(t, 0.f), 1.f);
                        q = (int)rintf(u * (float)OKN_ONE);
                    }
                    out = q > out ? min(out + rate, q) : max(out - rate, q);
                    const float lvl = (float)out / (float)OKN_ONE;
                    const float scaled = lvl * span;
                    a.raw[o] = av;
                    a.filtered[o] = f;
                    a.pose[o] = out;
                    a.angle[o] = lo + scaled;
                } else if (lane < OKF_MAXD) {                  // the columns from D on: zero
                    a.raw[o] = 0.f;
                    a.filtered[o] = 0.f;
                    a.pose[o] = 0;
                    a.angle[o] = 0.f;
                }
            }
        }
        __syncthreads();                                       // (sA is written again by the next batch)
    }
    if (wave == 0) {
        st->x[lane] = x;
        if (joint) st->out[lane] = out;
        if (lane == 0) st->started = started;
    }
}

struct OkfModelArgs {                    // what the host hands cp_online_kf_set_model's kernel
    int D;
    float lo[OKF_MAXD], span[OKF_MAXD];
    int rest[OKF_MAXD];
};

// the stream part of a state to its start: not started, x = 0, pose 0
__device__ __forceinline__ void okf_restart(OkfState* st, int tid) {
    if (tid < OKF_MAXS) st->x[tid] = 0.f;
    if (tid < OKF_MAXD) st->out[tid] = 0;
    if (tid == 0) st->started = 0;
}

// installs a model from device memory (W [D][512], b [D], M [2D][2D], K [2D][D]) and the host's lo, span and rest; the centre is
// c = lo + ((float) rest / 4096.f) * span; rows and columns past the model are zeroed and the stream restarts
__global__ __launch_bounds__(OKF_THREADS) void okf_set_model_kernel(OkfState* st, const float* __restrict__ W, const float* __restrict__ b,
                                                                    const float* __restrict__ M, const float* __restrict__ K, OkfModelArgs p) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, D = p.D, n2 = 2 * D;
    for (int e = tid; e < OKF_MAXD * OKN_F; e += OKF_THREADS) st->W[e] = e < D * OKN_F ? W[e] : 0.f;
    for (int e = tid; e < OKF_MAXS * OKF_MAXS; e += OKF_THREADS) {
        const int i = e / OKF_MAXS, j = e % OKF_MAXS;
        st->M[e] = i < n2 && j < n2 ? M[i * n2 + j] : 0.f;
    }
    for (int e = tid; e < OKF_MAXS * OKF_MAXD; e += OKF_THREADS) {
        const int i = e / OKF_MAXD, j = e % OKF_MAXD;
        st->K[e] = i < n2 && j < D ? K[i * D + j] : 0.f;
    }
    if (tid < OKF_MAXD) {
        const bool on = tid < D;
        const float lvl = (float)(on ? p.rest[tid] : 0) / (float)OKN_ONE;
        const float scaled = lvl * (on ? p.span[tid] : 0.f);
        st->b[tid] = on ? b[tid] : 0.f;
        st->lo[tid] = on ? p.lo[tid] : 0.f;
        st->span[tid] = on ? p.span[tid] : 0.f;
        st->rest[tid] = on ? p.rest[tid] : 0;
        st->c[tid] = on ? p.lo[tid] + scaled : 0.f;
    }
    if (tid == 0) st->D = D;
    okf_restart(st, tid);
}

// the stream part of streams first .. first + gridDim.x - 1 to its start; the model stays
__global__ __launch_bounds__(OKF_THREADS) void okf_reset_kernel(OkfState* states, int first) { okf_restart(states + first + blockIdx.x, threadIdx.x); }
