/* cpnative -- C ABI of the MI355X-native contrastive sEMG training path.
 *
 * The reference (FibonacciDude/ContrastiveProsthetics) is pure Python/PyTorch and has no
 * FFI layer; its de-facto operator boundary is the Python class surface of `Model`,
 * `EMGNet`, `GLOVENet` (code/models.py), `TaskWrapper` (code/utils.py), `DB23`
 * (code/load.py) and the step in `train_loop` (code/train.py:95-108).  Every entry point
 * below names the reference call site it replaces.  The library is what a maintainer binds
 * with ctypes from those classes; `contrastiveprosthetics_amd/` is
 * exactly such a binding.
 *
 * Conventions: plain pointers + sizes, no torch types.  All pointers are DEVICE pointers
 * unless the name ends in `_host`.  `stream` is a hipStream_t passed as void*.  Every call
 * only enqueues work on `stream`: no allocation, no synchronisation, no host read-back.
 * Return value: 0 on success, otherwise a hipError_t (or CP_ERR_* below); the message is
 * available from cp_last_error().  The library is gfx950-only and has no CPU fallback.
 *
 * Activations inside the workspace are stored in `dtype` (f32 = parity path computed with
 * v_mfma_f32_32x32x2_f32, bf16 = throughput path computed with v_mfma_f32_32x32x16_bf16 and
 * f32 accumulation); parameters, gradients, statistics, z, logits and the loss are f32.
 */
#ifndef CPNATIVE_H
#define CPNATIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CP_VERSION 112            /* 0.1.1: per-call state (cp_config carries options, tile schedule, sync-BN hook, gradient tap);
                                     111: cp_debug_gemm without its ablation argument;
                                     112: cp_config.record (cp_forward_record) */
#define CP_F32 0
#define CP_BF16 1
#define CP_FP8 2                  /* e4m3 activations and fc weights on the block-scaled MFMA (BASELINE config 4); see cp_config.dtype */
#define CP_TASKS 41               /* code/constants.py:45-48 */
#define CP_EMG_DIM 12             /* code/constants.py:97 */
#define CP_D_E 16                 /* embedding width (code/train.py:183) */
#define CP_N_BN 9                 /* 2 x BatchNorm2d(64) + 7 x BatchNorm1d(512) */
#define CP_N_FC 7
#define CP_ERR_ARG 10001
#define CP_ERR_WORKSPACE 10002

/* Pointers to the trainable tensors of `Model` (values) or to their gradients.
 * Shapes and state_dict keys: SURVEY.md section 8b / code/models.py:248-315, 412-428. */
typedef struct cp_params {
    float* conv1_w;            /* emg_net.conv_emg.0.weight (64,1,3,3) */
    float* conv1_b;            /* emg_net.conv_emg.0.bias   (64)       */
    float* conv2_w;            /* emg_net.conv_emg.3.weight (64,64,3,3)*/
    float* conv2_b;            /* emg_net.conv_emg.3.bias   (64)       */
    float* fc_w[CP_N_FC];      /* emg_net.linear.{0,3,6,9,13,17,21}.weight (512,768 | 512,512) */
    float* fc_b[CP_N_FC];      /* ...bias (512) */
    float* bn_g[CP_N_BN];      /* BN gamma: conv_emg.{2,5}, linear.{2,5,8,11,15,19,23} */
    float* bn_b[CP_N_BN];      /* BN beta */
    float* last_w;             /* emg_net.last.0.weight (16,512), no bias */
    float* easy_w;             /* glove_net.easy.0.weight (16,41) */
    float* easy_b;             /* glove_net.easy.0.bias   (16)    */
} cp_params;

/* running statistics of the stock nn.BatchNorm (code/models.py:238-243); all NULL for AdaBN
 * (code/models.py:17-35: momentum 0, track_running_stats False). */
typedef struct cp_bn_buffers {
    float* running_mean[CP_N_BN];
    float* running_var[CP_N_BN];
} cp_bn_buffers;

/* Synchronised-BatchNorm hook (see cp_config.stats_allreduce below): adds one row of `count` floats over all ranks in place. */
typedef int (*cp_allreduce_fn)(void* user, void* row_dev, int64_t count, void* stream);

/* Test / measurement switches of one call (cp_config.options; all 0 in production).  They select orders or forms of the SAME
 * computation that tests compare.  The library has no process-wide switch and reads no environment variable. */
#define CP_OPT_UNFUSED_BN_BWD 1u  /* BatchNorm + ReLU backward as its own pass behind every data gradient (the f32 path's order, on the bf16 kernels) */
#define CP_OPT_UNPAIRED_WGRAD 2u  /* one weight-gradient launch per layer behind a dropout instead of paired launches */
#define CP_OPT_FP8_BRIDGE 4u      /* CP_FP8: expand the saved 8-bit tensors to bf16 and run the bf16 backward kernels */
#define CP_OPT_NO_SMALL 8u        /* batches of <= 64 groups on the large-batch kernels instead of the small-batch form */
#define CP_OPT_FP8_HEAD_F32 16u   /* CP_FP8: the head's logits from the f32 matrix instruction instead of the block-scaled 8-bit one */
#define CP_OPT_FINALIZE_LAUNCHES 32u /* every bn_bwd_finalize and slab fold as a launch of its own (no finalisation in a consumer's prologue, no paired slab fold): same bits */

/* How the persistent fc GEMM kernels hand their output tiles to the CUs (cp_config.tile_schedule).  CP_TILES_STATIC: each
 * workgroup owns a fixed list of tiles -- fastest when this process has the GPU to itself (weight-stationary kernels).
 * CP_TILES_DYNAMIC: workgroups draw tiles from per-XCD counters -- 2-4 % slower alone, but a launch that shares CUs with
 * another stream's or process's kernels (a packed sweep, collectives that stay resident for long) no longer waits for its
 * latest-starting workgroup (+35 % with 8-32 CUs held).  BatchNorm partial sums are grouped per sample tile in the dynamic
 * mode and per workgroup in the static one, so the two differ in the last bits; each is run-to-run reproducible.
 * (The dynamic schedule's tile counters live in a module-global device table with one slot per stream; two streams never
 * share a slot.) */
enum { CP_TILES_STATIC = 0, CP_TILES_DYNAMIC = 1 };

/* What the last cp_encoder_forward left in a workspace (cp_config.record).  The caller allocates it in HOST memory, zeroes it and
 * keeps one per workspace buffer (a new buffer gets a new, zeroed record); the library reads and writes it only inside the calls.
 * cp_encoder_forward fills it; cp_encoder_backward reads it and counts itself in `backwards`. */
typedef struct cp_forward_record {
    int64_t n_windows;   /* the forward's n_windows; 0 = no forward has filled this record */
    int32_t path;        /* the forward's kernel path: 0 large-batch, 1 small-batch, 2 CP_FP8 */
    int32_t backwards;   /* backward passes run over this forward so far */
    int32_t transposed;  /* 1: the forward made the backward's transposed weights on cp_config.aux_stream */
    int32_t pad;
    void* join_event;    /* transposed: the forward's aux_join (a hipEvent_t recorded behind those transposes), else NULL */
} cp_forward_record;

/* Everything a call depends on besides its tensors.  Process-wide in the library are only: the thread-local error string of
 * cp_last_error; the opt-in profiler of cp_profile_enable (one profiled stream at a time); the out-of-range row count of
 * cp_gather_groups (see cp_gather_oob_count); and, for CP_TILES_DYNAMIC only, the tile counters of the persistent fc GEMM kernels,
 * one device slot per stream (see cp_config.tile_schedule).  Everything else lives in the caller's cp_config, workspace and
 * cp_forward_record: two engines (two cp_config / workspace / record triples) in one process, on one or several streams, do not
 * see each other.  A cp_encoder_backward call consumes the workspace of the cp_encoder_forward that filled its `record`: the
 * library checks that its config has the forward's n_windows and takes the forward's kernel path (dtype, and for 16/32 bits
 * whether the batch runs the small-batch form) and returns CP_ERR_ARG otherwise.  Nothing else in the config is checked. */
typedef struct cp_config {
    int64_t n_windows;   /* rows through the encoder = groups * 41 (train: B*41, eval: B*41*25) */
    int32_t dtype;       /* CP_F32 | CP_BF16 | CP_FP8 (the first F8_STATE_BYTES = 1024 bytes of a CP_FP8 workspace hold the tensors' scales across
                          * steps: zero them once after allocating it, and copy them into a buffer that replaces it, as
                          * contrastiveprosthetics_amd.engine.Engine.workspace does when it grows the workspace) */
    int32_t adabn;       /* 1: batch statistics in train AND eval (AdaBN); 0: stock BN */
    int32_t training;    /* 1: model.train()  (batch stats, dropout, running-stat update) */
    uint32_t step_state_lo; /* low / high half of the DEVICE address of a cp_step_state, or 0/0 (see below) */
    float dp_emg;        /* Dropout p after BN of fc4..fc7 (code/models.py:282-297) */
    float bn_momentum;   /* 0.1 */
    float bn_eps;        /* 1e-5 */
    uint32_t step_state_hi;
    uint64_t seed;       /* dropout stream = f(seed, step, layer, element) */
    uint64_t step;
    uint32_t options;    /* CP_OPT_* bits; 0 in production */
    int32_t tile_schedule;   /* CP_TILES_STATIC (0, default) | CP_TILES_DYNAMIC */
    /* ---- synchronised BatchNorm (opt-in: NULL = every rank normalises with its own shard's statistics, which is
     * the reference at B_local, code/models.py:17-35,238-243).  With a hook, every BatchNorm of the sEMG encoder takes its
     * batch statistics -- and, in the backward pass, the two sums of BatchNorm's data gradient -- over ALL ranks: the library
     * folds its partial sums into one row of `count` floats in the workspace and calls stats_allreduce(stats_user, row, count,
     * stream), which must add the rows of all ranks in place, ordered after the work already on `stream` and before what is
     * enqueued on it next (torch.distributed.all_reduce on that memory does exactly this).  stats_world = number of ranks (the
     * element count is scaled by it).  gamma / beta gradients stay this rank's part, as in torch.nn.SyncBatchNorm.  18 calls
     * per training step. */
    cp_allreduce_fn stats_allreduce;
    void* stats_user;
    int32_t stats_world;
    int32_t reserved0;
    /* ---- test aid: while grad_tap is non-NULL, cp_encoder_backward copies every intermediate gradient into it (stream-ordered):
     * 9 slots of n_windows x 768 elements of the compute dtype; slot L = 2..8: dL/d(pre-activation of fc layer L-1), i.e. after
     * BatchNorm + ReLU backward, n_windows x 512; slot 1: dL/d(conv2 pre-activation), slot 0: dL/d(BN1 output), both
     * n_windows x [12 positions][64 channels].  grad_tap_bytes = size of the buffer.  (Slot 0 is no tensor of the step since round 4 --
     * conv2's data gradient is consumed in the accumulators of conv2_dgrad_conv1_kernel -- so with a tap the call runs the stand-alone
     * data-gradient kernel once more to fill it; CP_FP8: slots 0 and 1 hold the bf16 expansion of the e5m2 gradient.)
     * The small-batch form (n_windows <= 2,624 with batch statistics) stores other tensors -- each launch applies the BatchNorm + ReLU
     * backward of ITS layer while staging its input -- and fills 11 slots: slot L = 2..8: the masked dL/d(BN_L output) (BN_L = the
     * BatchNorm behind fc layer L-1; dropout mask and 1 / (1 - p) applied, rounded to the compute dtype), n_windows x 512, i.e. the
     * gradient BEFORE layer L's BatchNorm + ReLU backward; slot 9: the same for conv2's BatchNorm, n_windows x 768 as fc1's launch
     * wrote it ([position][channel]); slot 1: dL/d(conv2 pre-activation), which conv2's weight-gradient launch writes over that
     * tensor in place; slot 0 as above; slot 10: dL/dz as cp_head stored it, n_windows x 64 with 16 live columns.
     * A tap never changes which kernels compute the step: it adds the copies and slot 0's stand-alone launch, and the second stream
     * (below) stays off.  The buffer's size is checked before the first launch (9 slots, small-batch form 11; CP_FP8 slots are
     * bf16): a short one returns CP_ERR_ARG with nothing enqueued. */
    void* grad_tap;
    size_t grad_tap_bytes;
    /* ---- a second stream for the work of cp_encoder_backward that nothing in the step waits for (round 4; all three NULL = one
     * stream, which is what contrastiveprosthetics_amd.engine passes by default: since the projection's and conv2's weight gradients
     * carry BatchNorm-backward sums they are on the critical path, and with only fc5..fc7's left to float one stream measured
     * faster -- DESIGN.md 7j).  The weight gradients of the layers behind a dropout (fc5..fc7) are not on the step's
     * critical path -- their BatchNorm-backward sums come from the data-gradient launches -- while ~40 latency-bound finaliser /
     * fold / reduction launches of the critical path leave most of the chip idle.  With aux_stream (a hipStream_t, ideally of
     * LOWER priority than `stream`) those weight-gradient launches and their slab reductions are enqueued there: aux_fork (a
     * hipEvent_t owned by the caller) is recorded on `stream` and waited for on aux_stream wherever a launch's inputs become
     * final, aux_join is recorded on aux_stream and waited for on `stream` before the call returns (and before fc_grads_ready is
     * recorded), so the caller sees the same stream-ordered semantics as without it.  Same kernels; fc5's and fc4's weight gradients are then summed over
     * 64 row splits each instead of 32 (alone instead of in one paired launch): equal to the rounding of an f32 sum, run-to-run exact.
     * Used by the large-batch 16- and 8-bit paths when dp_emg > 0; ignored elsewhere (f32, small batches, synchronised BatchNorm,
     * a gradient tap).  A training forward pass with it makes the backward's transposed weights on aux_stream and records aux_join
     * behind them (cp_forward_record.join_event): the backward over that forward waits for this event on `stream` before its
     * first launch, whether or not its own config uses the second stream. */
    void* aux_stream;
    void* aux_fork;
    void* aux_join;
    /* ---- the cp_forward_record of this workspace (above): filled by cp_encoder_forward when non-NULL, required by
     * cp_encoder_backward, consulted by cp_debug_activation when non-NULL; ignored by every other call */
    cp_forward_record* record;
} cp_config;

/* Per-step values kept in DEVICE memory so that a whole training step can be captured in a HIP graph and replayed
 * (graphs bake kernel arguments; these are the arguments that change from step to step).  The host refreshes the
 * 32 bytes with one asynchronous copy before each replay.  When cp_config.step_state_{lo,hi} hold its address, the
 * dropout stream is f(seed, layer, element) ^ dp_salt (cfg->step is then taken as 0), and cp_l2_adam_step_graph
 * reads the bias corrections and learning rates from it. */
typedef struct cp_step_state {
    uint32_t dp_salt;     /* any function of the step index, e.g. a hash of it */
    float bc1, bc2;       /* 1 - beta1^t, 1 - beta2^t */
    float lr_emg, lr_glove;
    uint32_t aug_salt;    /* the salt of this step's cp_gather_groups_aug, when its cp_augment names this state */
    float pad[2];
} cp_step_state;

int cp_version(void);
const char* cp_last_error(void);

/* bytes of scratch needed by the calls below for up to `max_windows` encoder rows */
size_t cp_workspace_bytes(int64_t max_windows, int32_t dtype, float dp_emg);

/* TaskWrapper.__getitem__ + DB23.__getitem__/slice_batch + default_collate
 * (code/utils.py:51-64, code/load.py:256-273, code/train.py:86,95) in one launch.
 * table: DB23.EMG_use (table_rows,12) f32 (eval: the same memory viewed as (rows/25,25,12));
 * emg_rand: TaskWrapper.emg_rand (41,D) int64; perm: the B item indices of this batch;
 * x_out: (B,41,V,12) f32 -- the collated EMG tensor in encoder row order. */
int cp_gather_groups(const float* table, int64_t table_rows, const int64_t* emg_rand, int64_t D,
                     const int64_t* perm, int64_t B, int32_t V, float* x_out, void* stream);
/* cp_gather_groups reads a source row outside [0, table_rows) from row 0 (the reference would raise an IndexError at
 * code/load.py:262-266) and counts it; this copies the running count of such rows since the last reset into the DEVICE
 * word count_out (stream-ordered) and, with reset != 0, zeroes it afterwards.  Non-zero = emg_rand, V and the table
 * do not belong together. */
int cp_gather_oob_count(uint32_t* count_out, int32_t reset, void* stream);

/* ---- sEMG augmentation in the gather (an opt-in EXTENSION of the data path, no reference counterpart) ---------------
 * cp_gather_groups_aug is cp_gather_groups -- same source rows, same out-of-range rule and counter, same single launch --
 * whose windows are perturbed before they are stored, in this order, for item i = item_offset + b*41 + t, sample v,
 * model channel d:
 *   1. ring shift: s uniform in shift_min..shift_max; channels 0..7 read source channel c = (d + s) mod 8, channels 8..11
 *      c = d (the map cp_online_*push_mapped takes for a sleeve turned by s positions);
 *   2. gain: G = exp(gain_sigma n_d) exp(amp_sigma n_i).  With mean_std the gain acts on the raw RMS value and the result
 *      is normalised with the model channel's constants, as a mapped push does: r = x[c] std[c] + mean[c],
 *      y = (r G - mean[d]) / std[d]; a channel with c == d and G == 1 keeps x[d] itself.  Without (NULL): y = x[c] G;
 *   3. noise: y += noise_sigma n per element, in normalised units;
 *   4. dead electrodes: channel d stores `fill` for the whole item with probability p_drop, or always if bit d of
 *      dead_mask is set.
 * Shift, gains and the dead set are drawn per item: the V windows of an evaluation item share them.  Every draw is a
 * counter-based function of (seed, salt, i, v, d) -- csrc/kernels_misc.cuh states the chain, and
 * contrastiveprosthetics_amd/augment.py restates it in numpy -- so a window's perturbation does not depend on B, the
 * grid or the launch.  f32 arithmetic in the order above, contraction off.  A setting that is off draws nothing; with
 * everything off x_out is cp_gather_groups' output bit for bit.
 * salt: per gather, any function of a step counter.  salt_state_{lo,hi}: the DEVICE address of a cp_step_state, or 0/0;
 * when set, the kernel reads the salt from its aug_salt word instead (graph replay).
 * Refused with CP_ERR_ARG before anything is enqueued: what cp_gather_groups refuses, a table or x_out that is not 16-byte aligned, a NULL aug, shift bounds outside
 * -7..7 or min > max, p_drop outside [0, 1], a sigma that is negative, not finite or above 2, a `fill` that is not
 * finite, dead_mask above 0xFFF, item_offset below 0 or item_offset + B*41 above 2^32.  Allocates, synchronises and
 * reads nothing. */
typedef struct cp_augment {
    uint32_t seed, salt;
    uint32_t salt_state_lo, salt_state_hi;
    int32_t shift_min, shift_max;
    uint32_t dead_mask;
    float p_drop, gain_sigma, amp_sigma, noise_sigma, fill;
    const float* mean_std;      /* (24) device floats: [d] mean, [12 + d] std of the raw RMS value; or NULL */
    int64_t item_offset;
} cp_augment;
int cp_gather_groups_aug(const float* table, int64_t table_rows, const int64_t* emg_rand, int64_t D,
                         const int64_t* perm, int64_t B, int32_t V, float* x_out, const cp_augment* aug, void* stream);

/* EMGNet.forward (code/models.py:319-342): conv_emg -> linear -> last.
 * x (n_windows,12) f32, 16-byte aligned (a window's 12 values are read as three 16-byte loads; cp_gather_groups'
 * output and any torch allocation are); z_out (n_windows,16) f32 in the same row order (the regroup of
 * models.py:337-341 is a pure index map applied by cp_head).  Saves what backward needs in ws. */
int cp_encoder_forward(const cp_config* cfg, const cp_params* p, const cp_bn_buffers* bn,
                       const float* x, void* ws, size_t ws_bytes, float* z_out, void* stream);

/* Model.forward's normalise + bmm with GLOVENet.forward's one-hot Linear
 * (code/models.py:121-130, 457-465), Model.loss / contrastive_loopy_loss
 * (code/models.py:132-173, 198-208) and their gradient, fused.
 * labels (B*41) int64; n_groups = B*V; loss_correct[0] = loss, [1] = number of rows whose
 * argmax equals its label; pred (n_groups,41) int32; logits optional (n_groups,41,41) f32.
 * want_grad: also writes dL/dz into ws (consumed by cp_encoder_backward) and the class-encoder
 * gradients grads->easy_w / easy_b.
 * Position j of group g carries the class embedding of labels[(g / V)*41 + j]; the targets of both loss directions and
 * of loss_correct[1] are labels[0..40] for every group (code/models.py:147), which need not be a permutation.
 * n_groups must be a multiple of V and z 16-byte aligned (CP_ERR_ARG otherwise, as in cp_head_gneg). */
int cp_head(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels,
            int64_t n_groups, int32_t V, int32_t want_grad, void* ws, size_t ws_bytes,
            float* loss_correct, int32_t* pred, float* logits, cp_params* grads, void* stream);

/* ---- global negatives (an opt-in EXTENSION of the loss, no reference counterpart) ---------------------
 * The reference's class->EMG direction (code/models.py:136-147 on the transposed logits) is a softmax over the 41 windows
 * of ONE group.  With this extension the column of class k of group b ranges over its positive window and every window
 * of another class in the GLOBAL batch (all groups of all ranks):
 *     col[b,k] = -s[b,pos_k,k] + log( exp(s[b,pos_k,k]) + G[k] ),   G[k] = sum_{all windows n, class(n) != k} exp(s[n,k])
 * z_all (n_all_windows,16) f32: the z embeddings of the global batch in window order (the RCCL all-gather of every rank's
 * cp_encoder_forward output; at one rank, that output itself); labels (>= 41) int64: class of position t of a group.
 * gh_out: 128 device floats {G[64], H[64]} (41 used each; H[k] = sum over all groups of 1/(exp(pos) + G[k]) carries the
 * gradient into the negatives).  scratch: cp_global_negatives_scratch_floats(n_all_windows) device floats.
 * cp_head_gneg = cp_head with that table: row direction unchanged, column direction as above; gradients are those of
 * this rank's windows (the data-parallel gradient sum adds the ranks' parts).  One-hot class table, training batches.
 * The extension is defined for the identity layout, labels[t] = t: under another layout the table's kernels and the head
 * mean different rows by a column's "positive". */
size_t cp_global_negatives_scratch_floats(int64_t n_all_windows);
int cp_global_negatives(const cp_params* p, const float* z_all, int64_t n_all_windows, const int64_t* labels,
                        float* scratch, float* gh_out, void* stream);
int cp_head_gneg(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels,
                 int64_t n_groups, int32_t V, int32_t want_grad, void* ws, size_t ws_bytes,
                 float* loss_correct, int32_t* pred, float* logits, cp_params* grads, const float* gh, void* stream);
/* The same table WITHOUT moving z: the class table is replicated, so G and H are sums of per-rank terms and only two 41-float
 * vectors have to cross ranks.  cp_global_negatives_g: this rank's rows' part of G into gh[0..63]; the caller sums gh[0..63] over
 * the ranks (one all-reduce of 64 floats); cp_global_negatives_h: with the summed G in place, this rank's groups' part of H into
 * gh[64..127]; the caller sums that too.  scratch as above for n_local_windows, kept between the two calls (it holds the positives).
 * cp_global_negatives on the gathered rows == _g, sum, _h, sum on each rank's own rows (tests/test_gpu_global_batch.py). */
int cp_global_negatives_g(const cp_params* p, const float* z_local, int64_t n_local_windows, const int64_t* labels,
                          float* scratch, float* gh, void* stream);
int cp_global_negatives_h(int64_t n_local_windows, const int64_t* labels, float* scratch, float* gh, void* stream);


/* autograd of EMGNet (what loss.backward() does at code/train.py:105 for emg_net):
 * consumes dL/dz left in ws by cp_head, writes every emg_net gradient into `grads`.  cfg->record must be the record that
 * the forward over ws filled (CP_ERR_ARG if it is NULL, was never filled, or names another n_windows or kernel path); a
 * repeated backward over one forward gives the same gradients. */
int cp_encoder_backward(const cp_config* cfg, const cp_params* p, const float* x, void* ws,
                        size_t ws_bytes, cp_params* grads, void* stream);
/* The same, for data-parallel training: `fc_grads_ready` (a hipEvent_t, or NULL) is recorded on `stream` as soon as every
 * gradient except the conv stack's (conv1, its BatchNorm, conv2, its BatchNorm -- 0.15 of the 8.1 MB) is final, about
 * 0.5 ms before the call's last kernel at 167,936 windows: the caller's all-reduce of that part (torch.distributed /
 * RCCL on another stream, after a wait on the event) runs beside the conv backward.  No reference counterpart: the
 * reference is single-process (code/train.py:105). */
int cp_encoder_backward_ev(const cp_config* cfg, const cp_params* p, const float* x, void* ws,
                           size_t ws_bytes, cp_params* grads, void* stream, void* fc_grads_ready);

/* eval majority vote (code/models.py:151-163): pred (B,V,41) -> curve (B,V) of prefix-mode
 * accuracies, y_pred (B,41) = mode over all V samples. */
int cp_vote(const int32_t* pred, const int64_t* labels, int64_t B, int32_t V, float* curve,
            int32_t* y_pred, void* stream);

/* Class-subset evaluation for MANY subsets in one launch.  The reference's product
 * use-case (README.md:11-19): at test time the user keeps a subset S of the 41 classes; only the EMG rows t in S
 * and the class-encoding columns c in S of every 41 x 41 logits tile take part,
 *     pred[b,v,t] = argmax_{c in S} logits[b*V+v, t, c]            (code/models.py:147, first maximum wins)
 * followed by the prefix majority vote of code/models.py:151-163 (torch.mode: ties -> smallest class id).
 * logits (B*V,41,41) f32 as Model.forward returns them in eval (what results.py:45 saves as logs.npy);
 * labels (41) int64 = labels[:tasks]; masks (n_masks,41) uint8 (non-zero = member);
 * correct (n_masks,V) int64 OVERWRITTEN with the number of (b, t in S) whose mode over the first w+1 samples
 * equals labels[t] (accuracy = correct / (B*|S|); Model.voting_raw lays w = 0..V-1 out over win = 1..249);
 * y_pred optional (n_masks,B,41) int32: mode over all V samples, -1 for rows outside S (results.py:51).
 * V <= 64. */
int cp_subset_vote(const float* logits, const int64_t* labels, int64_t B, int32_t V, const uint8_t* masks,
                   int64_t n_masks, int64_t* correct, int32_t* y_pred, void* stream);

/* sklearn.metrics.confusion_matrix(y_true, y_pred) of code/results.py:58 as counts:
 * counts (41,41) int64 += 1 at [labels[i % 41]][y_pred[i]] for i < n_groups*41; y_pred < 0 is skipped. */
int cp_confusion(const int32_t* y_pred, const int64_t* labels, int64_t n_groups, int64_t* counts, void* stream);

/* Raw-sEMG preprocessing = DB23.get_stim_rep after the slice (code/load.py:102-109) with
 * utils.filter / utils.rms (code/utils.py:137-156), for all segments at once.
 * raw (n_segments, seg_len, 12) f32 on the device: the first seg_len = 2000 + 2*5 samples of each
 * (stimulus, repetition) mask, as scipy.io.loadmat delivers `emg` (float32).  b, a: HOST pointers to the n_coef <= 17
 * IIR coefficients (scipy.signal.butter(4, (20, 450)/1000, "bandpass") in the reference); gain = 2**10;
 * rms_window = 11; time_idx: HOST pointer to the n_out <= 256 kept positions of the RMS series
 * (load.py:115 time_mask, whose uint8 wraps modulo 256 -- pass what the reference computes).
 * out (n_segments, n_out, 12) f32.  Rounding points follow NumPy/SciPy exactly: bit-identical samples.
 * Accepted range: rms_window <= seg_len <= 2**31 - 17; every time_idx[i] in 0 .. n_rms - 1 with
 * n_rms = seg_len - 2 * (rms_window / 2), in any order, repeats allowed.  Positions are 32-bit from here to the
 * kernel, so a segment may be a whole recording.  Anything else is CP_ERR_ARG before a launch. */
int cp_preprocess_emg(const float* raw, int64_t n_segments, int32_t seg_len, const double* b, const double* a,
                      int32_t n_coef, int32_t rms_window, float gain, const int32_t* time_idx, int32_t n_out,
                      float* out, void* stream);

/* utils.RunningStats over preprocessed segments (code/utils.py:79-135; load.py:116,141-144): statistics of the
 * per-segment channel means of the segments with use[s] != 0 (use == NULL: all) -- their mean and sample standard
 * deviation per channel, or averaged over channels when complete != 0.  scratch: n_segments*12 doubles on the
 * device.  mean_std (2,12) f32 on the device. */
int cp_emg_stats(const float* seg, int64_t n_segments, int32_t n_out, const uint8_t* use, int32_t complete,
                 double* scratch, float* mean_std, void* stream);

/* RunningStats.normalize (code/utils.py:134, load.py:148): seg = (seg - mean) / std in place, f32. */
int cp_emg_normalize(float* seg, int64_t n_rows, const float* mean_std, void* stream);

/* ---- glove-angle class encoder (BASELINE config 3) -------------------------------------
 * zg = last(relu(BN(Linear(20->256, no bias)(glove)))), last = Linear(256->16, no bias): the layers the reference
 * keeps as comments in GLOVENet (code/models.py:386-391, 461) plus its built-but-unused `self.last`
 * (code/models.py:425-428).  One row per (group, class).  The contrastive head then takes row (b*41 + j) of zg as
 * the class embedding of position j of group b, instead of the one-hot table's row labels[b*41 + j]. */
typedef struct cp_glove_params {
    float* w1;            /* glove_net.linear.1.weight        (256,20) */
    float* bn_g;          /* glove_net.linear.2[.bn].weight   (256) */
    float* bn_b;          /* glove_net.linear.2[.bn].bias     (256) */
    float* last_w;        /* glove_net.last.0.weight          (16,256) */
    float* running_mean;  /* stock BN buffers (NULL under AdaBN; unused in a gradient struct) */
    float* running_var;
} cp_glove_params;

size_t cp_glove_workspace_bytes(int64_t max_rows, int32_t dtype);

/* GLOVENet.forward, glove branch.  glove (rows,20) f32, rows = B*41; zg (rows,16) f32.  cfg supplies dtype, adabn,
 * training, bn_momentum, bn_eps (n_windows and the dropout fields are not used).  Saves what backward needs in gws.
 * glove and zg must be 16-byte aligned (CP_ERR_ARG otherwise). */
int cp_glove_forward(const cp_config* cfg, const cp_glove_params* gp, const float* glove, int64_t rows,
                     void* gws, size_t gws_bytes, float* zg, void* stream);

/* cp_head with per-group class embeddings: same outputs; want_grad (V must be 1) leaves dL/dz in ws for
 * cp_encoder_backward and dL/dzg in gws for cp_glove_backward.  z and zg must be 16-byte aligned (CP_ERR_ARG otherwise). */
int cp_head_glove(const cp_config* cfg, const float* z, const float* zg, const int64_t* labels, int64_t n_groups,
                  int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, void* gws, size_t gws_bytes,
                  float* loss_correct, int32_t* pred, float* logits, void* stream);

/* ---- learnable temperature (an opt-in EXTENSION of the loss: the CLIP ingredient the reference leaves switched off) ----
 * logit_scale: ONE device float s (read on the stream, so a replayed graph sees what the optimiser left there).  With
 * S = ln 100 and tau = exp(min(max(s, -S), S)):
 *     logits[g][i][j] = tau * z_hat[g,i] . E_hat[label(g,j)]        (the logits that come back are the scaled ones)
 * loss, loss_correct[1], pred and the vote are cp_head's functions of those logits (pred does not depend on tau).  With
 * dl = dL/dlogits formed on the scaled logits:
 *     dz_hat = tau * dl E_hat,   dE_hat = tau * dl^T z_hat,
 *     dL/ds  = sum_{g,i,j} dl[g,i,j] * logits[g,i,j]  for -S <= s <= S, and 0 outside that range.
 * With 8-bit logits (CP_FP8 without "fp8_head_f32") the gradient products keep the f32 operands (straight-through) and
 * dL/ds sums dl times the quantised, scaled logit.
 * cp_head_temp / cp_head_glove_temp = cp_head / cp_head_glove with that factor: same arguments, outputs and refusals, plus
 * logit_scale (NULL: CP_ERR_ARG) and d_logit_scale (one device float, written when want_grad; NULL with want_grad:
 * CP_ERR_ARG).  At s = 0 every output equals the twin's bit for bit.  There is no global-negatives twin: its {G, H} table
 * would need tau as well.  cp_debug_head_grad / cp_debug_glove_head_grad read what these calls left. */
int cp_head_temp(const cp_config* cfg, const cp_params* p, const float* z, const int64_t* labels,
                 int64_t n_groups, int32_t V, int32_t want_grad, void* ws, size_t ws_bytes,
                 float* loss_correct, int32_t* pred, float* logits, cp_params* grads,
                 const float* logit_scale, float* d_logit_scale, void* stream);
int cp_head_glove_temp(const cp_config* cfg, const float* z, const float* zg, const int64_t* labels, int64_t n_groups,
                       int32_t V, int32_t want_grad, void* ws, size_t ws_bytes, void* gws, size_t gws_bytes,
                       float* loss_correct, int32_t* pred, float* logits,
                       const float* logit_scale, float* d_logit_scale, void* stream);

/* autograd of the glove encoder: consumes dL/dzg left in gws, writes w1, bn_g, bn_b, last_w of `grads`. */
int cp_glove_backward(const cp_config* cfg, const cp_glove_params* gp, int64_t rows, void* gws, size_t gws_bytes,
                      cp_glove_params* grads, void* stream);

/* Model.l2() (code/models.py:225-228, 344-349, 467-472) + optimizer_emg.step() +
 * optimizer_glove.step() (code/train.py:72-73, 101, 107-108) over one flat parameter buffer.
 * Tensor table (host arrays, n <= 64): offset/numel into the flat buffers, group (0 emg_net,
 * 1 glove_net), l2 (1 if the tensor's name contains neither 'bn' nor 'bias').
 * step_index: 1-based Adam step.  grad_scale multiplies the data gradient (1/world_size after an
 * all-reduce sum).  l2_out: device scalar receiving the regulariser value.  scratch: device floats,
 * at least cp_optimizer_scratch_floats(...) long.
 * Per element, with n = |p| the Frobenius norm of the element's tensor:
 *     g' = grad_scale * g + reg * p / n        (members of the regulariser; the second term is 0 where n = 0)
 *     m  = beta1 * m + (1 - beta1) * g',   v = beta2 * v + (1 - beta2) * g'^2
 *     p  = p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * A member whose norm is 0 (a zero-initialised or pruned tensor) takes no regulariser gradient -- torch.norm's gradient at the
 * zero tensor is 0 -- and follows its data gradient; it adds 0 to the regulariser value.
 * Any table of 1..64 entries that do not overlap is taken, entries of no element included; the flat buffers need no alignment
 * (a tensor whose offset and numel are multiples of 4 is read in 16-byte pieces where the four base pointers are 16-byte
 * aligned, every other tensor element by element: the same numbers either way).  Nothing outside the table's elements is written.
 * Refused with CP_ERR_ARG and a cp_last_error that names the entry, before any launch: n outside 1..64, a negative offset or
 * numel, a table without an element, a NULL pointer, step_index < 1. */
typedef struct cp_adam_hyper {
    float lr_emg, lr_glove, reg_emg, reg_glove;
    float beta1, beta2, eps, grad_scale;
} cp_adam_hyper;
/* cp_l2_adam_step with lr_emg, lr_glove and the bias corrections read from a device cp_step_state (graph replay);
 * the other fields of h are used as given. */
int cp_l2_adam_step_graph(float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq,
                          const int64_t* offset_host, const int64_t* numel_host, const int32_t* group_host,
                          const int32_t* l2_host, int32_t n, const cp_adam_hyper* h, const cp_step_state* state_dev,
                          float* scratch, float* l2_out, void* stream);
size_t cp_optimizer_scratch_floats(const int64_t* numel_host, int32_t n);
int cp_l2_norms(const float* params_flat, const int64_t* offset_host, const int64_t* numel_host,
                const int32_t* group_host, const int32_t* l2_host, int32_t n, const cp_adam_hyper* h,
                float* scratch, float* l2_out, void* stream);
int cp_l2_adam_step(float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq,
                    const int64_t* offset_host, const int64_t* numel_host, const int32_t* group_host,
                    const int32_t* l2_host, int32_t n, const cp_adam_hyper* h, int64_t step_index,
                    float* scratch, float* l2_out, void* stream);

/* Optional timing of kernel groups with HIP events recorded on the launch stream (used by
 * bench.py for the live roofline figure).  cp_profile_enable creates the events (never done inside
 * a step); every profiled launch group then records a start/stop pair until max_records are used.
 * cp_profile_summary (after the caller synchronised the stream) sums the elapsed times of one kind. */
enum {
    CP_K_GATHER = 0, CP_K_PREP = 1, CP_K_CONV1_FWD = 2, CP_K_BN_FINALIZE = 3, CP_K_CONV2_FWD = 4,
    CP_K_FOLD = 5, CP_K_FC_FWD = 6, CP_K_DROPOUT = 7, CP_K_PROJ_FWD = 8, CP_K_HEAD = 9,
    CP_K_PROJ_BWD = 10, CP_K_BN_BWD = 11, CP_K_FC_WGRAD = 12, CP_K_REDUCE_SLABS = 13,
    CP_K_FC_DGRAD = 14, CP_K_CONV2_WGRAD = 15, CP_K_CONV2_DGRAD = 16, CP_K_CONV1_BWD = 17,
    CP_K_OPT = 18, CP_K_FC_DGRAD_STATS = 19, CP_K_FC_DGRAD_BN = 20,
    CP_K_FC_FWD_WS = 21,         /* forward fc launches that ran the weight-stationary kernel (K = 512: fc2..fc7) */
    CP_K_FC_DGRAD_CONV = 22,     /* CP_FP8: fc1's data gradient (16-bit output for the conv kernels) -- its own kernel instantiation */
    CP_K_COUNT = 23
};
int cp_profile_enable(uint64_t kind_mask, int32_t max_records);
int cp_profile_disable(void);
/* records again after cp_profile_disable, keeping what was recorded (sampling every n-th step: each recorded launch costs
 * two event records, ~5 us of idle queue apiece) */
int cp_profile_resume(void);
int cp_profile_summary(int32_t kind, double* total_ms, int64_t* count);

/* debug/test access: copy saved activation `layer` (0..8 = post-ReLU pre-BN output of conv1,
 * conv2, fc1..fc7; rows x C in the internal layout, conv layers position-major [w][c]; 9..12 =
 * dropout(BN(.)) of fc4..fc7, present only when dp_emg > 0 and the forward ran in training) to f32.
 * Layer 0 (conv1) is never stored by the forward pass -- its consumers recompute it from x -- so it
 * is recomputed here the same way from `p` and `x` (both may be NULL for the other layers).  Layers 9..11 are read as the
 * forward's kernel path stored them: the path of cfg->record when it is non-NULL and filled, else the path `cfg` selects. */
int cp_debug_activation(const cp_config* cfg, const cp_params* p, const float* x, void* ws,
                        size_t ws_bytes, int32_t layer, float* out, void* stream);
/* test aid: `blocks` workgroups of 256 threads that each hold a CU's LDS (so nothing else fits next to them there) and spin
 * for about `microseconds` -- stands in for another stream's kernel (an RCCL collective) competing for CUs. */
int cp_debug_hog(int32_t blocks, int32_t microseconds, void* stream);
/* micro-benchmark access (tools/gemm_bench.py): one fc-layer GEMM launch on caller buffers.
 * kind 0: forward   C[M][F] = relu(A[M][K] W[F][K]^T + bias), column sums -> partials
 * kind 1: data grad C[M][F] = A[M][K] W[F][K]^T, sums against R[M][F] -> partials
 * kind 2: weight grad slabs[S][P][Q] = sum_m X[m][P] Y[m][Q]   (A = X, W = Y, K = P, F = Q) */
int cp_debug_gemm(int32_t dtype, int32_t kind, int64_t M, int32_t K, int32_t F, const void* A,
                  const void* W, void* C, const float* bias, const void* R, float* partials,
                  void* stream);
/* debug/test access (tests/test_gpu_fc_gemm_exact.py): every fc-layer GEMM launch on caller buffers, one at a time.  cp_debug_gemm
 * is this entry with CP_TILES_STATIC and no coef / dropout.  lda = K, ldc = ldr = F.  What runs (CP_BF16; CP_F32 runs the 128-tile
 * parity kernels under either schedule and takes neither coef nor dropout):
 *   kind 0                        static: the weight-stationary forward (K = 512; K = 768 with F = 512), else the persistent kernel;
 *                                 dynamic: the persistent kernel.  partials: rows of [2][F], column sums of C and C^2 as stored
 *   kind 1, R NULL                the persistent kernel, plain product, no sums (*stat_rows_out = 0)
 *   kind 1, R and coef            C = R > 0 ? ca (A W^T) + cb R + cz : 0 with ca / cb / cz[f] = coef[{0,1,2} * coef_mod + f % coef_mod];
 *                                 partials: rows of [F], column sums of C.  Static: weight-stationary (K = 512), dynamic: persistent
 *   kind 1, R without coef        C = mask (A W^T) dp_inv_keep (dp_thresh != 0: element (m, f) is kept when the 16-bit draw of the
 *                                 dropout hash of (dp_key, m, F, f) is >= dp_thresh), partials: rows of [2][F], column sums of C and
 *                                 C R.  Static: weight-stationary (K = 512), dynamic: persistent
 *   kind 2                        slabs[S][K][F] = sum over the rows of split s of A[m][K]^T W[m][F] (*stat_rows_out = S)
 * stat_rows_out (host, may be NULL): the number of partial rows written.  Under CP_TILES_DYNAMIC that is one row per 256-row
 * sample tile, in tile order; otherwise one row per worker of the kernel that ran.
 * Checked before anything launches, CP_ERR_ARG: NULL A / W / C (partials for kinds 0 and 1, bias for kind 0), M <= 0, K % 64, F % 256
 * (kind 2: K % 256, CP_F32 128), CP_BF16 kinds 0 and 1 with F > 768, an unknown dtype / kind / tile_schedule, M max(K, F) 2 >= 2^32 - 2^20,
 * R / coef / dropout outside kind 1, coef or dropout without R or outside CP_BF16, both at once, coef_mod <= 0 with coef,
 * dp_thresh > 65535, dp_inv_keep <= 0 with dropout, A / W / C / R not 16-byte aligned. */
typedef struct cp_debug_fc_gemm_args {
    int32_t dtype;             /* CP_F32 | CP_BF16 */
    int32_t kind;              /* 0 forward, 1 data gradient, 2 weight gradient */
    int64_t M;
    int32_t K;
    int32_t F;
    int32_t tile_schedule;     /* CP_TILES_STATIC | CP_TILES_DYNAMIC */
    int32_t coef_mod;
    const void* A;
    const void* W;
    void* C;
    const float* bias;
    const void* R;
    float* partials;
    const float* coef;         /* [3][coef_mod] or NULL */
    uint32_t dp_thresh;        /* 0: no dropout */
    uint32_t dp_key;
    float dp_inv_keep;
    int32_t reserved0;
    int32_t* stat_rows_out;
} cp_debug_fc_gemm_args;
int cp_debug_fc_gemm(const cp_debug_fc_gemm_args* args, void* stream);

/* debug/test access (tests/test_gpu_conv_exact.py): every launch of the LARGE-batch conv front end on caller buffers, one step of
 * the pass at a time, at any n_windows (also below the 2,625 windows from which the step dispatches these kernels).  The kernels are
 * reached through the launch functions of the step (csrc/encoder_api.cuh): its grids, slab counts and pre-reduce rule.  T = float
 * (CP_F32) or bf16 (CP_BF16); rows = n_windows * 12, position-major [window][position][channel].
 *   kind 0   conv1_stats_kernel<T>: partials[g][2][64] = sum and sum of squares of r1 = round_T(relu(conv1(x))); *rows_out = g
 *   kind 1   prep_conv2_kernel<T>, conv2_strip_kernel<T, 0>: out[rows][64] = round_T(relu(conv2(s r1 + t) + conv2_b)) with
 *            s = stats1[2][.], t = stats1[3][.] (rows 0 and 1 of stats1 are not read); partials[grid][2][64] = sum and sum of
 *            squares of out as stored; *rows_out = grid
 *   kind 2   prep_conv2_kernel<T>, conv2_strip_kernel<T, 1>: out[rows][64] = round_T(conv2's data gradient of gin[rows][64]);
 *            partials[grid][2][64] = sum of out and of out * r1; *rows_out = grid
 *   kind 3   (colsum_kernel<T> -> partials[<= 256][768] when gcols is NULL,) conv2_wgrad_kernel<T> (gin_exp: <T, true>) -> slabs[S][64][192]
 *            = the raw product gin^T r1 of the strips s, s + S, ..; reduce_rows_kernel when S > 64 -> 32 folded slabs BEHIND slab S - 1;
 *            conv2_wgrad_finish_kernel<T> -> dw = dW2 (64,64,3,3), fold = rows2[64][2][64] (BatchNorm1's backward sums per output
 *            channel).  stats1 rows 2 and 3 are read.  *rows_out = S, *gcol_rows_out = rows of column sums the finish kernel read
 *   kind 4   prep_conv2_kernel<T>, conv2_dgrad_conv1_kernel<T> (gin_exp: <T, true>) -> partials[grid][4][64] (dW1 tap 0..2, db1) with
 *            gy = r1 > 0 ? ca g_v1 + cb r1 + cz : 0, ca / cb / cz = coef[0..2][.]; reduce_rows_kernel when grid > 64 -> fold[32][4][64];
 *            conv1_bwd_finalize_kernel -> dw = dW1 (64,1,3,3), db = db1[64].  *rows_out = grid
 * wc: scratch of 2 * 64 * 192 T that prep_conv2_kernel fills (kinds 1, 2, 4).  gin_exp (device int32, kinds 3 and 4 under CP_BF16):
 * gin holds e5m2 bytes, stored = value * 2^*gin_exp.  Every scratch region is the caller's, so guards behind the rows and slabs
 * a launch reports can be inspected.  rows_out / gcol_rows_out: host, may be NULL.
 * Checked before anything launches, CP_ERR_ARG: a NULL pointer the kind reads or writes, n_windows <= 0, an unknown dtype or kind,
 * gin_exp outside kinds 3 / 4 or CP_BF16, or in kind 3 without gcols (the step refuses that too), gcols with gcol_rows <= 0,
 * x / gin / gcols / wc / out / partials / slabs / fold not 16-byte aligned, n_windows * 768 * sizeof(T) >= 2^32 - 2^20 (the conv
 * kernels index in 64 bits; the bound is the step's, beyond which nothing has run them). */
typedef struct cp_debug_conv_args {
    int32_t dtype;             /* CP_F32 | CP_BF16 */
    int32_t kind;              /* 0..4 */
    int64_t n_windows;
    const float* x;            /* [n_windows][12] */
    const float* conv1_w;      /* (64,1,3,3) */
    const float* conv1_b;      /* [64] */
    const float* conv2_w;      /* (64,64,3,3), kinds 1..4 */
    const float* conv2_b;      /* [64], kind 1 */
    const float* stats1;       /* [4][64], kinds 1 and 3 */
    const void* gin;           /* [n_windows * 12][64] T or e5m2 bytes, kinds 2..4 */
    const int32_t* gin_exp;    /* device, or NULL */
    const float* gcols;        /* [gcol_rows][768] or NULL, kind 3 */
    const float* coef;         /* [3][64], kind 4 */
    void* wc;
    void* out;
    float* partials;
    float* slabs;
    float* fold;
    float* dw;
    float* db;
    int32_t gcol_rows;
    int32_t reserved0;
    int32_t* rows_out;
    int32_t* gcol_rows_out;
} cp_debug_conv_args;
int cp_debug_conv(const cp_debug_conv_args* args, void* stream);

/* debug/test access (tests/test_gpu_proj_exact.py): every launch sequence of the 512 -> 16 projection of the LARGE-batch step on
 * caller buffers, one at a time, at any row count M (no 41-window groups; also below the size from which the step dispatches these
 * kernels).  The kernels are reached through the launch functions of the step (csrc/encoder_api.cuh: launch_proj_fwd, proj_dz_sums,
 * launch_proj_wgrad_tn, launch_proj_wgrad_onepass, proj_sums_from_wgrad; csrc/gemm_ws.cuh: launch_proj_dgrad): its row splits,
 * grids and partial-row counts.  T = float (CP_F32) or bf16 (CP_BF16).  Wp (16, 512) f32 is the weight in the reference layout;
 * the entry runs the step's preparation kernels on it into caller scratch, so the zero padding they write is part of what runs.
 * act[M][512] is the saved post-ReLU activation r, dz[M][64] T the head's gradient (columns 16..63 zero), s = scale[512],
 * t = shift[512].  keep(m, f): the 16-bit draw of the dropout hash of (dp_key, m, 512, f) is >= dp_thresh.
 *   kind 0   forward, out = z[M][16] f32.  dp_thresh == 0: fold_linear_kernel<T> -> w32 = wlast[32][512] = round_T(Wp diag s), rows
 *            16..31 zero, blast[16] = Wp t; gemm_nt_kernel<T,128,32,ALOAD_PLAIN,EPI_PLAIN_F32> -> z = r wlast^T + blast.
 *            dp_thresh != 0: the plain copy (fold_copy_batch_kernel<T>, one job; with r_exp fold_linear_kernel<T> without s / t, as
 *            the CP_FP8 step) -> wlast = round_T(Wp), blast = 0; ALOAD_BNDROP -> z = round_T(keep (s r + t) dp_inv_keep) wlast^T.
 *            r_exp: ALOAD_F8 / ALOAD_BNDROP_F8
 *   kind 1   weight gradient, no dropout.  colsum_kernel<T>, colsum_finalize_kernel -> dzsum[16]; gemm_tn_kernel<T,64,128,YLOAD_PLAIN>
 *            (r_exp: YLOAD_F8) -> slabs[S][64][512]; reduce_slabs_kernel -> out = dW (16, 512) = s P + t dzsum with P = dz^T r
 *            -> praw[16][512]; bn_bwd_sums_from_wgrad_kernel -> partials[2][512] = sum_j Wp[j][.] dzsum[j], sum_j Wp[j][.] P[j][.]
 *            (the column sums of dz first pass through partials[<= 64][16]).  *rows_out = S
 *   kind 2   weight gradient behind a dropout, two products (CP_F32, or CP_BF16 under CP_OPT_UNFUSED_BN_BWD).
 *            gemm_tn_kernel<T,64,128,YLOAD_BNDROP> -> slabs[S][64][512]; reduce_slabs_kernel -> out = dW = dz^T u with
 *            u = round_T(keep (s r + t) dp_inv_keep).  *rows_out = S
 *   kind 3   the same gradient in one pass (CP_BF16).  proj_wgrad_sums_kernel<false> (r_exp: <true>) -> slabs[S][32][512], rows 0..15
 *            A = dz^T (keep r), rows 16..31 B = dz^T keep; proj_wgrad_finish_kernel -> out = dW = (s A 2^-r_exp + t B) dp_inv_keep
 *            and partials[4][2][512]: row y holds sum_j bf16(Wp[j][.]) B[j][.] and sum_j bf16(Wp[j][.]) A[j][.] (times dp_inv_keep,
 *            A in true units) over j = 4y..4y+3.  *rows_out = S
 *   kind 4   data gradient behind a dropout (CP_BF16).  transpose_w_kernel<bf16> -> w32 = wlast_t[512][64] = bf16(Wp)^T, columns 16..63
 *            zero; proj_dgrad_kernel -> out = C[M][512] bf16 = r > 0 ? ca g + cb r + cz : 0 with g = bf16(keep (dz wlast_t^T) dp_inv_keep),
 *            ca / cb / cz = coef[0..2][.]; partials[rows][512] = column sums of C as stored, one row per worker; *rows_out = rows as
 *            launch_proj_dgrad reports them
 * S = the splits of split_rows(M, 128 splits, 32-row steps).  w32: scratch of 32 * 512 T (kind 0) or 512 * 64 T (kind 4).  r_exp
 * (device int32, kinds 0, 1 and 3 under CP_BF16): act holds e4m3 bytes, stored = value * 2^*r_exp.  Every scratch and output region
 * is the caller's, so guards behind them can be inspected.  rows_out: host, may be NULL.
 * proj_dgrad8_kernel (csrc/fp8.cuh), the CP_FP8 step's data gradient, needs the 8-bit state block: cp_debug_fp8, kind 6.
 * Checked before anything launches, CP_ERR_ARG: a NULL pointer the kind reads or writes (Wp, act; dz for kinds 1..4; scale and
 * shift for kinds 0..3; coef for kind 4; w32 for kinds 0 and 4; blast for kind 0; out; slabs for kinds 1..3; partials for kinds 1, 3
 * and 4; praw and dzsum for kind 1), M <= 0, an unknown dtype or kind, kinds 3 and 4 or r_exp outside CP_BF16, r_exp in kinds 2 and
 * 4, dropout (dp_thresh, dp_key or dp_inv_keep non-zero) in kind 1, dp_key or dp_inv_keep non-zero with dp_thresh == 0 in kind 0,
 * no dropout (dp_thresh == 0) in kinds 2..4, dp_thresh > 65535, dp_inv_keep <= 0 with dropout, Wp / act / dz / w32 / out / slabs / partials / praw / scale / shift / coef / blast / dzsum not
 * 16-byte aligned, M * 512 * sizeof(T) >= 2^32 - 2^20 (the step's bound: 32-bit byte offsets and the hash's 32-bit element index). */
typedef struct cp_debug_proj_args {
    int32_t dtype;             /* CP_F32 | CP_BF16 */
    int32_t kind;              /* 0..4 */
    int64_t M;
    const float* Wp;           /* (16, 512) */
    const void* act;           /* [M][512] T or e4m3 bytes */
    const int32_t* r_exp;      /* device, or NULL */
    const void* dz;            /* [M][64] T, kinds 1..4 */
    const float* scale;        /* [512], kinds 0..3 */
    const float* shift;        /* [512], kinds 0..3 */
    const float* coef;         /* [3][512], kind 4 */
    void* w32;
    float* blast;              /* [32], kind 0 */
    void* out;
    float* slabs;
    float* partials;
    float* praw;               /* [16][512], kind 1 */
    float* dzsum;              /* [16], kind 1 */
    uint32_t dp_thresh;        /* 0: no dropout */
    uint32_t dp_key;
    float dp_inv_keep;
    int32_t reserved0;
    int32_t* rows_out;
} cp_debug_proj_args;
int cp_debug_proj(const cp_debug_proj_args* args, void* stream);

/* debug/test access (tests/test_gpu_fp8_exact.py): every launch of the 8-bit fc path (CP_FP8, csrc/fp8.cuh) on caller buffers, one
 * launch sequence at a time, at any row count M >= 1.  The kernels are reached through the launch functions and the grid and split
 * expressions of the step (csrc/fp8.cuh: launch_gemm_ws8, launch_gemm_wsd8, launch_gemm_tn8, launch_proj_dgrad8; csrc/encoder_api.cuh:
 * launch_bn_dropout_apply8, launch_bn_relu_bwd8, split_rows_tn8, launch_reduce_slabs8).  state is the caller's scale table: 1,024
 * device bytes laid out as Fp8State (int32 e[64], uint32 amax[64], uint32 init, padding): stored = value * 2^e[t], amax[t] the float
 * bits of the largest stored-unit magnitude before clamping.  A launch reads e[] of the ids it is given and raises amax[t_out].
 *   kind 0   launch_gemm_ws8<K> (K = 512 | 768, F = 512): C[M][F] e4m3 = clamp(relu(A[M][K] W[F][K]^T 2^(wsc[f] - 127) + bias[f]), 448);
 *            partials[rows][2][F] = column sums of the clamped values and of their squares, one row per worker (partials NULL: the
 *            evaluation form, no sums); amax[t_out] = the largest accumulator
 *   kind 1   launch_gemm_wsd8<0> (F = 512 | 768): C[M][F] e5m2 = R > 0 ? ca' acc + cb' R + cz' : 0 with acc = A[M][512] (e5m2) W[F][512]^T
 *            2^(wsc[f] - 127), ca' = ca 2^eo, cb' = cb 2^(eo - er), cz' = cz 2^eo, ca / cb / cz[f] = coef[{0,1,2} * coef_mod + f % coef_mod],
 *            eo = e[t_out], er = e[t_r], R[M][F] e4m3; partials[rows][F] = column sums of C as stored, in true units
 *   kind 2   launch_gemm_wsd8<1> (F = 512): C = R != 0 ? acc dp_inv_keep 2^eo : 0 (R = a dropout output u); partials[rows][2][F] =
 *            sum g (true units) and sum g r derived from sum g u through bn_stats[4][F] (mean, invstd, scale, shift)
 *   kind 3   launch_gemm_tn8, reduce_slabs_kernel<bf16>: slabs[S][512][F] bf16 = the products A[m][512]^T (e5m2) R[m][F] (e4m3) of the
 *            rows of split s, C = dW[512][F] f32 = their sum times 2^-(e[t_in] + e[t_r]).  A2 / R2 / partials2 / C2 / t_in2 / t_r2: a
 *            second problem in the same launch (F = 512, 32 splits each; its slabs lie in partials2).  partials = the slabs
 *   kind 4   launch_bn_dropout_apply8: C[M][512] e4m3 = keep ? (s A 2^-e[t_in] + t) dp_inv_keep 2^e[t_out] : 0 with s / t = bn_stats[2 / 3][.]
 *   kind 5   launch_bn_relu_bwd8, in place: C[M][512] e5m2 (t_in) -> R > 0 ? ca' g + cb' R + cz' : 0 (t_out), ca' = ca 2^(eo - e[t_in]);
 *            partials[rows][512] = column sums as stored, true units, one row per block
 *   kind 6   launch_proj_dgrad8: C[M][512] e5m2 = R > 0 ? ca' g + cb' R + cz' : 0, g = keep (A[M][64] bf16 W[512][64]^T bf16) dp_inv_keep
 *            (dp_thresh == 0: no mask); partials[rows][512]
 *   kind 7   weight preparation of one layer from A = W[512][K] f32 (mode 0 | 1: fold_linear8_kernel, mode 1 = fc1's order k' = w*64 + c,
 *            scale / shift NULL or the previous BatchNorm's affine; C = weight bytes [512][K], wsc[512], partials = bias[512] in output
 *            units, t_out < 0: f32 output;  mode 2 | 3: transpose_w8_batch_kernel with one job, mode 3 = fc1's order; C = [K][512], wsc[K],
 *            t_in = the gradient's id)
 *   kind 8   fp8_update_scales_kernel on state with n_windows = M
 * keep(m, f): the 16-bit draw of the dropout hash of (dp_key, m, 512, f) is >= dp_thresh.  *rows_out (host, may be NULL): partial rows
 * written (kinds 0..2, 5, 6), splits (kind 3), else 0.
 * Checked before anything launches, CP_ERR_ARG: a NULL pointer the kind reads or writes, M <= 0, a shape the launch functions refuse
 * (kind 0: K 512 | 768 and F 512; kinds 1, 3: F 512 | 768; kinds 2, 4..6: F 512; kind 3 paired: F 512; kind 7: K 512 | 768), an
 * unknown kind or mode, a pointer not 16-byte aligned, an id outside 0..63 (kind 7: t_out may be -1), coef_mod <= 0 in kind 1,
 * dp_thresh > 65535, dp_inv_keep <= 0 where it is read, M max(K, F) >= 2^32 - 2^20. */
typedef struct cp_debug_fp8_args {
    int32_t kind;              /* 0..8 */
    int32_t mode;              /* kind 3: 1 = paired; kind 7: 0..3 */
    int64_t M;
    int32_t K;
    int32_t F;
    int32_t coef_mod;
    int32_t t_in;
    int32_t t_r;
    int32_t t_out;
    int32_t t_in2;
    int32_t t_r2;
    void* state;               /* 1,024 bytes, Fp8State */
    const void* A;
    const void* W;
    const void* wsc;
    const float* bias;
    const void* R;
    const float* coef;
    const float* bn_stats;
    const float* scale;        /* kind 7 */
    const float* shift;
    void* C;
    float* partials;
    const void* A2;            /* kind 3, paired */
    const void* R2;
    float* partials2;
    float* C2;
    uint32_t dp_thresh;        /* 0: no dropout */
    uint32_t dp_key;
    float dp_inv_keep;
    int32_t reserved0;
    int32_t* rows_out;
} cp_debug_fp8_args;
int cp_debug_fp8(const cp_debug_fp8_args* args, void* stream);

/* debug/test access (tests/test_gpu_bn_exact.py): the f32 / bf16 BatchNorm and weight-preparation launches that sit between the GEMMs
 * of the large-batch step (csrc/kernels_misc.cuh) on caller buffers, one launch sequence at a time, at any row count >= 1.  The kernels
 * are reached through the launch functions of the step (csrc/encoder_api.cuh: PreReduce, launch_bn_finalize, launch_running_stats,
 * launch_eval_folds, launch_bn_bwd_finalize, launch_bn_dropout_apply, launch_bn_relu_bwd, launch_bias_grad_from_rows,
 * launch_fold_linear, launch_fold_copies, launch_weight_transposes): its grids, caps, job tables and pre-reduce rule.  T = float
 * (CP_F32) or bf16 (CP_BF16) where the kernel is templated (kinds 1, 3, 4, 5; kinds 0 and 2 are f32 throughout and ignore dtype
 * beyond its check).  M is the number of partial rows in kinds 0 and 2, the number of activation rows in kinds 3 and 4.
 *   kind 0   statistics.  rows = partials[M][2][C] (sum, sum of squares), C = 64 | 512.  PreReduce (reduce_rows_kernel into
 *            scratch[32][2C] when M > 2,048) then bn_finalize_kernel -> stats[4][C] = mean, invstd, scale = gamma invstd, shift =
 *            beta - mean scale, from mean = s1 / count, var = max(s2 / count - mean^2, 0), invstd = 1 / sqrt(var + eps); update_running
 *            != 0: running_mean / running_var (both non-NULL then) <- (1 - momentum) old + momentum (mean | var count / (count - 1)).
 *            unscale_exp (device int32 or NULL): s1 is scaled by 2^-e and s2 by 2^-2e first.
 *   kind 1   evaluation prologue.  launch_running_stats on the nine tables params->bn_g / bn_b, bn->running_mean / running_var
 *            (C = 64, 64, 512 x 7) -> stats9[l][4][C]; then the eight-job fold_linear_batch_kernel<T> as the evaluation forward fills
 *            it: fc1 (params->fc_w[0], K = 768, mode 1: stored k' = w*64 + c of k = c*12 + w) .. fc7 folded with the affine of the
 *            BatchNorm below each -> wimg[i][512][K] T = W diag s, bimg[i][512] = b + W t; the projection params->last_w (16, 512),
 *            no bias -> wimg[7][32][512] T (rows 16..31 zero), bimg[7][16] = W t
 *   kind 2   backward coefficients.  rows = partials[M][2][C nfold] (sum g, sum g r; feature f*C + c belongs to channel c), (C, nfold) =
 *            (512, 1) | (64, 1) | (64, 12).  PreReduce (into scratch[32][2 C nfold] when M > 2,048) then bn_bwd_finalize_kernel with
 *            stats[4][C] -> coef[3][C], dgamma[C], dbeta[C].  local (or NULL): one row [2][C nfold]; dgamma / dbeta then come from it
 *   kind 3   bn_dropout_apply_kernel<T> on the step's grid: g = u[M][512] T = keep ? (s r + t) dp_inv_keep : 0 with r[M][512] T,
 *            s / t = stats[2 | 3][.], keep(m, f): the 16-bit draw of the dropout hash of (dp_key, m, 512, f) is >= dp_thresh
 *   kind 4   bn_relu_bwd_kernel<T> in place, then launch_bias_grad_from_rows.  C = 512 (cap CAP_BRB16) | 64 (cap 2,048):
 *            g[M][C] T <- r > 0 ? ca g + cb r + cz : 0 with ca / cb / cz = coef[0..2][.]; partials[gb][C] = per-block column sums
 *            of g as stored; db[C] = their sum; *rows_out = gb
 *   kind 5   weight preparation during training.  mode 0 | 1: launch_fold_linear<T> in that mode on W (512, K) f32, K = 512 | 768
 *            (mode 1: K = 768), b[512], s / t (both or neither; NULL: the plain copy) -> wimg[0][512][K] T, bimg[0][512].  mode 2: the
 *            four-job fold_copy_batch_kernel<T> as the dropout forward fills it -> wimg[4..6], bimg[4..6] (fc5..fc7), wimg[7][32][512],
 *            bimg[7][16] = 0 (projection).  mode 3: the eight-job transpose_w_batch_kernel<T> as the backward fills it ->
 *            wimg[i][K][512] T = W^T (fc1 in the order k' = w*64 + c), wimg[7][512][64] T = last_w^T, columns 16..63 zero
 * Every scratch and output region is the caller's, so guards behind them can be inspected.  rows_out: host, may be NULL.
 * Checked before anything launches, CP_ERR_ARG: a NULL pointer the kind reads or writes (params' and bn's members included), M <= 0
 * (kinds 0, 2, 3, 4), count < 1 (kinds 0, 2), an unknown dtype, kind, mode or shape (C, nfold, K), s without t, update_running without
 * running buffers, a pointer not 16-byte aligned, dp_thresh > 65535 or dp_inv_keep <= 0 in kind 3,
 * M * C * sizeof(T) >= 2^32 - 2^20 in kinds 3 and 4 (the step's bound), M >= 2^31 in kinds 0 and 2 (partial rows are counted in 32 bits). */
typedef struct cp_debug_bn_args {
    int32_t dtype;             /* CP_F32 | CP_BF16 */
    int32_t kind;              /* 0..5 */
    int32_t mode;              /* kind 5: 0..3, else 0 */
    int32_t C;                 /* kinds 0, 2, 4: 64 | 512 */
    int32_t nfold;             /* kind 2: 1 | 12 */
    int32_t K;                 /* kind 5, modes 0 and 1: 512 | 768 */
    int32_t update_running;    /* kind 0 */
    int32_t reserved0;
    int64_t M;
    double count;              /* kinds 0, 2 */
    float momentum;            /* kind 0 */
    float eps;                 /* kinds 0, 1 */
    uint32_t dp_thresh;        /* kind 3 */
    uint32_t dp_key;
    float dp_inv_keep;
    int32_t reserved1;
    const float* rows;         /* kinds 0, 2: the partial rows */
    const float* gamma;        /* [C], kind 0 */
    const float* beta;
    float* running_mean;       /* [C] or NULL, kind 0 */
    float* running_var;
    const int32_t* unscale_exp; /* device, or NULL, kind 0 */
    float* scratch;            /* kinds 0, 2, 4: the pre-reduce's 32 rows */
    float* stats;              /* [4][C]: out in kind 0, in in kinds 2 and 3 */
    const float* local;        /* [2][C nfold] or NULL, kind 2 */
    float* coef;               /* [3][C]: out in kind 2, in in kind 4 */
    float* dgamma;             /* [C], kind 2 */
    float* dbeta;
    const void* r;             /* [M][C] T, kinds 3, 4 */
    void* g;                   /* [M][C] T: u in kind 3, the gradient in kind 4 */
    float* partials;           /* [gb][C], kind 4 */
    float* db;                 /* [C], kind 4 */
    const cp_params* params;   /* kinds 1, 5 (modes 2, 3): device pointers in a host struct */
    const cp_bn_buffers* bn;   /* kind 1 */
    const float* W;            /* kind 5, modes 0 and 1 */
    const float* b;
    const float* s;            /* or NULL */
    const float* t;
    float* stats9[CP_N_BN];    /* kind 1 */
    void* wimg[CP_N_FC + 1];   /* kinds 1, 5 */
    float* bimg[CP_N_FC + 1];
    int32_t* rows_out;
} cp_debug_bn_args;
int cp_debug_bn(const cp_debug_bn_args* args, void* stream);

/* BN statistics of `layer` as computed by the last forward: out[4][C] = mean, invstd, scale, shift */
int cp_debug_bn_stats(const cp_config* cfg, void* ws, size_t ws_bytes, int32_t layer, float* out,
                      void* stream);

/* debug/test access to the head's data gradients.  cp_debug_head_grad: the n_windows x 64 rows of dL/dz that the last
 * cp_head / cp_head_gneg / cp_head_glove call with want_grad left in ws (window order as z; columns 0..15 live, 16..63 the zeros
 * the projection's backward kernels contract over), widened to f32 into out (n_windows*64 floats).  cp_debug_glove_head_grad:
 * the rows x 64 rows of dL/dzg that cp_head_glove left in gws, likewise.  cfg / ws / gws as for those calls; a NULL out is
 * CP_ERR_ARG, a short workspace CP_ERR_WORKSPACE.  One conversion launch each; nothing in the workspace changes. */
int cp_debug_head_grad(const cp_config* cfg, void* ws, size_t ws_bytes, float* out, void* stream);
int cp_debug_glove_head_grad(const cp_config* cfg, void* gws, size_t gws_bytes, int64_t rows, float* out, void* stream);

/* ---- online grasp decoding (README.md:11-19 of the reference: a prosthetic hand reads a live sEMG stream) ----------------
 * Consecutive chunks of raw 2 kHz, 12-channel sEMG -> for every 10 ms window a chunk completes, the predicted class and the
 * class voted over the last `vote` predictions.  Per sample: the transform of cp_preprocess_emg (gain 2**10, the IIR b/a,
 * float64 RMS sum over 11 samples with the 'nearest' start) and cp_emg_normalize, carried across calls; window k is the RMS-series
 * position phase + 20 k, final once raw sample phase + 20 k + 10 has arrived, and bit-identical to cp_preprocess_emg +
 * cp_emg_normalize of the whole recording at that position.  Then the sEMG encoder in eval mode with running-statistics
 * BatchNorm folded into the layer behind each BN (f32 or bf16), z / |z| against a table of K <= 64 L2-normalised class rows,
 * argmax (first maximum) and the mode of the vote ring (ties: smallest class id).
 * The library keeps no state: the filter, RMS history, sample count, vote ring, class table and folded weights live in the
 * workspace; the caller keeps the config and passes it to every call.  A push of n samples emits
 *     M = c(n_seen + n) - c(n_seen),  c(N) = max(0, floor((N - phase + 9) / 20))
 * windows (n_seen = samples pushed since the last reset), so the caller sizes the outputs without reading the device. */
#define CP_ONLINE_MAX_CLASSES 64
#define CP_ONLINE_MAX_VOTE 256
#define CP_ONLINE_MAX_WINDOWS 256     /* windows per push (the tail launch keeps their predictions in LDS) */
#define CP_ONLINE_STRIDE 20      /* raw samples per window (2 kHz -> 100 Hz) */
typedef struct cp_online_config {
    int32_t dtype;           /* CP_F32 | CP_BF16 */
    int32_t max_windows;     /* windows one push may emit: a push takes at most 20 * max_windows samples */
    int32_t vote;            /* length of the vote ring, 1..256 (25 = 250 ms, code/constants.py:74-78) */
    int32_t phase;           /* 0..19 */
    int32_t n_coef;          /* IIR coefficients, 2..17 (the reference's band-pass: 9) */
    int32_t reserved0;
    double b[17], a[17];     /* host values, as for cp_preprocess_emg */
} cp_online_config;

/* bytes of the workspace for up to max_windows_per_push windows per push (cp_online_config.max_windows).  A fresh workspace
 * must be zeroed (or cp_online_reset) before the first push. */
size_t cp_online_workspace_bytes(int32_t max_windows_per_push, int32_t dtype);
/* folds the model's parameters (f32, as for cp_encoder_forward) into the workspace in the compute dtype: BN1 -> conv2 (the
 * shift is position-dependent at the two edge positions: zero padding), BN2 -> fc1, BN_l -> fc_{l+1}, BN9 -> projection.
 * bn must hold all running statistics: AdaBN (bn == NULL) is refused with CP_ERR_ARG.  Pushes use this copy until the next
 * call. */
int cp_online_prepare(const cp_online_config* cfg, const cp_params* p, const cp_bn_buffers* bn, float bn_eps, void* ws,
                      size_t ws_bytes, void* stream);
/* table (n_classes,16) f32 (normalised here), ids (n_classes) int32 ascending: the class id each row reports.  Empties the vote
 * ring; the filter state stays. */
int cp_online_set_classes(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* table, const int32_t* ids,
                          int32_t n_classes, void* stream);
/* raw (n_samples,12) f32 -> pred, voted (M) int32 class ids; logits (M,n_classes) f32 and windows (M,12) f32 (the normalised
 * windows) may be NULL.  mean_std (2,12) f32: the normalisation of the training data (cp_emg_stats). */
int cp_online_push(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                   const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, void* stream);
/* zeroes the stream part of the state (filter, RMS history, sample count, vote ring); class table and weights stay */
int cp_online_reset(const cp_online_config* cfg, void* ws, size_t ws_bytes, void* stream);

/* ---- adaptive online decoding: BatchNorm unfolded, per-stream statistics (AdaBN calibration and drift tracking) ----------
 * The same decoder with the 9 BatchNorms kept unfolded.  For BN b (layer order) and channel c the workspace holds float64
 * (mu, v); P = the values one window gives a channel: 12 for BN1 and BN2 (positions, as BatchNorm2d pools them), 1 for
 * BN3..BN9.  With x_1..x_P the channel's pre-BN values of window t, m their mean and w their biased variance, a push runs
 * the windows in stream order and, for each BN in layer order:
 *     y = gamma (x - mu) / sqrt(v + eps) + beta                    with the statistics before window t, then
 *     d = m - mu,  mu <- mu + alpha d,  v <- (1 - alpha)(v + alpha d^2) + alpha w
 * (the exact moments of the mixture with weights (1 - alpha, alpha); alpha = 0 freezes the statistics; alpha is per window,
 * 100 Hz, so the time constant is about 1 / (100 alpha) s).  conv2 zero-pads the normalised conv1 output.  The recurrence is
 * serial in float64 in a fixed order and the GEMMs sum fixed-order tiles, so pred, voted, logits and the statistics after a
 * push are bit-identical for any chunking.
 * The workspace begins with the state of the folded form: cp_online_set_classes and cp_online_reset take an adaptive
 * workspace (reset keeps the statistics); cp_online_prepare and cp_online_push do not. */
size_t cp_online_adapt_workspace_bytes(int32_t max_windows_per_push, int32_t dtype);
/* copies the model's parameters (f32, as for cp_online_prepare) into the workspace in the compute dtype, unfolded, with
 * gamma, beta, bn_eps and alpha in [0, 1).  bn != NULL: the statistics become the running statistics (mu = running_mean,
 * v = running_var, what eval mode uses); bn == NULL (AdaBN, or a refresh of the weights): the statistics stay as they are,
 * which on a fresh (zeroed) workspace means uncalibrated -- the caller must not push before cp_online_adapt_calibrate. */
int cp_online_adapt_prepare(const cp_online_config* cfg, const cp_params* p, const cp_bn_buffers* bn, float bn_eps, double alpha,
                            void* ws, size_t ws_bytes, void* stream);
/* bytes of the caller-owned scratch of a calibration over n_windows windows */
size_t cp_online_adapt_calibrate_scratch_bytes(int64_t n_windows, int32_t dtype);
/* windows (n_windows >= 2, 12) f32, normalised as a push's windows are: sets every (mu, v) to the batch statistics of the
 * windows -- mean and biased variance over n_windows * P values -- layer by layer, each layer normalised with its own final
 * statistics before the next layer's are taken (the reference's AdaBN in eval, models.py:17-35, on that batch).  float64
 * (n, mean, M2) per chunk of <= 256 windows are merged in a fixed order.  Leaves the stream state, vote ring and class
 * table alone. */
int cp_online_adapt_calibrate(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows,
                              void* scratch, size_t scratch_bytes, void* stream);
/* as cp_online_push, on an adaptive workspace; updates the statistics by the workspace's alpha */
int cp_online_adapt_push(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                         const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, void* stream);
/* out (9, 2, 512) float64 on the device: mu, v of each BN (the conv BNs fill channels 0..63, the rest is zero) */
int cp_online_adapt_statistics(const cp_online_config* cfg, void* ws, size_t ws_bytes, double* out, void* stream);

/* ---- multi-stream online decoding: n_streams <= 256 streams, one model, one chain of launches per push -----------------
 * The decoder of cp_online_* with the folded weights stored once and one state (filter, RMS history, sample count, vote ring,
 * class table) per stream.  All streams share cfg (dtype, vote, phase, IIR; cfg.max_windows bounds the windows ONE stream
 * emits in a push) and mean_std.  Every call takes n_streams and max_rows, the windows one push may emit over all streams
 * (1..65536), as the workspace was sized with.  A push takes the samples of all streams packed in stream order: raw
 * (total_samples, 12), counts (n_streams) int32 on the device, counts[s] >= 0 samples of stream s.  Stream s emits
 *     M_s = c(n_seen_s + counts[s]) - c(n_seen_s)
 * windows (c as for cp_online_push), total_windows = sum M_s <= max_rows; its outputs are the rows row0_s = M_0 + .. + M_{s-1}
 * .. row0_s + M_s - 1 of pred, voted (total_windows) int32, logits (total_windows, 64) f32 (columns >= the stream's class
 * count are not written) and windows (total_windows, 12), and equal bit for bit those of cp_online_push on a workspace of that
 * stream alone fed the same chunks.  The caller sizes the outputs from its own sample counts: nothing is read back.  A stream
 * whose counts disagree with total_samples, total_windows or cfg.max_windows is left untouched (its outputs are not written).
 * A push is ten launches for any n_streams (front end, conv2, fc1..fc7, tail); none when total_samples is 0. */
#define CP_ONLINE_MULTI_MAX_STREAMS 256
#define CP_ONLINE_MULTI_MAX_ROWS 65536
size_t cp_online_multi_workspace_bytes(int32_t n_streams, int32_t max_rows, int32_t dtype);
/* as cp_online_prepare: folds the weights once for all streams */
int cp_online_multi_prepare(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, const cp_params* p,
                            const cp_bn_buffers* bn, float bn_eps, void* ws, size_t ws_bytes, void* stream);
/* as cp_online_set_classes, for stream `index` (0..n_streams-1) */
int cp_online_multi_set_classes(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                int32_t index, const float* table, const int32_t* ids, int32_t n_classes, void* stream);
/* as cp_online_reset, for stream `index`, or every stream for index -1 */
int cp_online_multi_reset(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                          int32_t index, void* stream);
int cp_online_multi_push(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                         const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                         const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, void* stream);

/* ---- adaptive multi-stream online decoding: cp_online_adapt_* for n_streams <= 256 streams in one chain per push ----------
 * The streams of cp_online_multi_* with the BatchNorms of cp_online_adapt_* kept unfolded.  The unfolded weights, gamma and
 * beta are stored once; each stream has its own state (as cp_online_multi_*), its own alpha in [0, 1) and eps, and its own
 * float64 statistics (9, 2, 512), which the recurrence of cp_online_adapt_* updates window by window in stream order.  Calls
 * take n_streams and max_rows as the cp_online_multi_* ones do; packing, counts, outputs and untouched streams are as for
 * cp_online_multi_push.  Every stream's pred, voted, logits, windows and statistics after a push equal bit for bit those of a
 * cp_online_adapt_* workspace with that stream's alpha, statistics, class table and state fed the same chunks.  A push is
 * twelve launches for any n_streams (front end, BN1, conv2, BN2, fc1..fc7, tail); none when total_samples is 0.
 * The workspace begins as a cp_online_multi_* workspace of the same n_streams and max_rows: cp_online_multi_set_classes and
 * cp_online_multi_reset take it (reset keeps the statistics and alpha); cp_online_multi_prepare and cp_online_multi_push do
 * not.  A fresh (zeroed) workspace has alpha 0 on every stream. */
size_t cp_online_multi_adapt_workspace_bytes(int32_t n_streams, int32_t max_rows, int32_t dtype);
/* as cp_online_adapt_prepare, once for all streams: copies the weights, gamma, beta and conv1 unfolded and sets every stream's
 * eps.  bn != NULL: every stream's statistics become the running statistics; bn == NULL: they stay (AdaBN, or a refresh).
 * alpha: n_streams host values in [0, 1), stream s's alpha; NULL: every alpha stays (cp_online_multi_adapt_set_alpha changes
 * one). */
int cp_online_multi_adapt_prepare(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, const cp_params* p,
                                  const cp_bn_buffers* bn, float bn_eps, const double* alpha, void* ws, size_t ws_bytes,
                                  void* stream);
/* alpha in [0, 1) of stream `index` from the next push on (0 freezes its statistics) */
int cp_online_multi_adapt_set_alpha(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                    int32_t index, double alpha, void* stream);
/* the statistics of stream `index` only: bn != NULL: the running statistics (as cp_online_multi_adapt_prepare); bn == NULL:
 * zero, as on a fresh workspace (uncalibrated: the caller must not push samples to it before calibrating it) */
int cp_online_multi_adapt_reset_statistics(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws,
                                           size_t ws_bytes, int32_t index, const cp_bn_buffers* bn, void* stream);
/* cp_online_adapt_calibrate of stream `index` against the shared weights; scratch of cp_online_adapt_calibrate_scratch_bytes.
 * No other stream's statistics, and no stream's state, vote ring or class table, change. */
int cp_online_multi_adapt_calibrate(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                    int32_t index, const float* windows, int64_t n_windows, void* scratch, size_t scratch_bytes,
                                    void* stream);
/* as cp_online_multi_push, on an adaptive multi-stream workspace */
int cp_online_multi_adapt_push(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                               const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                               const float* mean_std, int32_t* pred, int32_t* voted, float* logits, float* windows, void* stream);
/* out (9, 2, 512) float64 on the device: the statistics of stream `index`, laid out as cp_online_adapt_statistics */
int cp_online_multi_adapt_statistics(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                     int32_t index, double* out, void* stream);

/* ---- class enrolment: per-user class rows (cosine prototypes) for the online decoders, without a gradient ----------------
 * The logits of a decoder are cosines z^ . E^_c, so the row that serves one user best for class c is the mean direction of
 * that user's own z^ = z / |z| over windows of c.  Enrolment takes a labelled recording of the user, sums z^ per class into a
 * caller-owned accumulator and blends the summed directions with the rows the decoder has.
 * Windows and labels.  A recording is raw (n,12) f32 with one label per raw sample: a class id, or a negative value for "not
 * labelled".  It is a fresh stream of its own (cp_online_windows on a zeroed state): the decoder's filter state, sample count
 * and vote ring are not touched.  Window k (RMS-series position phase + 20 k) covers the raw samples phase + 20 k ..
 * phase + 20 k + 10; it takes their label if all 11 carry the same non-negative label, else it is skipped.  The caller maps
 * labels to slots: slot = position of the class id in the ascending id list of cp_online_set_classes.
 * Embedding.  z of a window is what the decoder's own push computes for it: the folded weights (cp_online_enroll,
 * cp_online_multi_enroll), or the unfolded weights with the stream's current statistics frozen, whatever its alpha
 * (cp_online_adapt_enroll, cp_online_multi_adapt_enroll); enrolment never moves statistics.  The layers run through the
 * device functions of the push, a row's value does not depend on the tile, chunk or call it falls in, and z^ is
 * z / sqrtf(sum z^2) in f32 as in the push's tail.
 * Accumulator.  acc (64,17) float64 on the device, zeroed by the caller before the first call: per slot 16 sums of z^ (the
 * f32 values widened) and the window count.  Every (slot, dimension) sum takes one float64 add per window, in window order
 * (no atomics, no reduction across workgroups), so acc after any sequence of calls depends only on the sequence of (window,
 * slot) pairs, not on how it was cut into calls or chunks.  Windows whose slot lies outside 0..n_classes-1 are skipped.
 * Several recordings accumulate into one acc.
 * Table.  With E^_c = prior_c / |prior_c| (f32, as cp_online_set_classes normalises) and S_c the sums of slot c, a slot with
 * count >= min_windows and |S_c| > 0 gets the direction (1 - mix) E^_c + mix S_c / |S_c|, mix in [0, 1], computed in float64
 * and written at the prior's length, table_c = (1 - mix) prior_c + mix |prior_c| S_c / |S_c|; every other slot gets prior_c.
 * So mix = 0, and a slot that is not enrolled, return prior_c bit for bit, and cp_online_set_classes of `table` (which
 * normalises the rows and empties the vote ring) then reproduces the row the decoder had exactly.  A zero prior row has no
 * direction: its row is S_c / |S_c| alone (a class the decoder did not have).
 * None of these entries allocates, synchronises or keeps state in the library; each validates on the host and returns
 * CP_ERR_ARG before anything is enqueued. */
/* bytes of the caller-owned front-end state of cp_online_windows; zero it to start a recording */
size_t cp_online_frontend_state_bytes(void);
/* the front end of a push alone (one launch): raw (n_samples,12) f32, at most 20 * cfg.max_windows samples, the next chunk of the
 * recording whose state (256-byte aligned) the caller holds -> the c(n_seen + n_samples) - c(n_seen) windows the chunk
 * completes, (M,12) f32 from row 0 of `windows`, bit-identical to those of cp_online_push */
int cp_online_windows(const cp_online_config* cfg, void* state, size_t state_bytes, const float* raw, int64_t n_samples,
                      const float* mean_std, float* windows, void* stream);
/* bytes of the caller-owned scratch of an accumulate call over n_windows windows (the activations of one chunk of <= 256) */
size_t cp_online_enroll_scratch_bytes(int64_t n_windows, int32_t dtype);
/* windows (n_windows,12) f32 as a push makes them, slots (n_windows) int32, acc (64,17) float64: adds the windows to acc in
 * order, in chunks of <= 256 windows (8 encoder launches and ole_accumulate_kernel per chunk; the adaptive forms 10 and
 * ole_accumulate_kernel).  n_windows == 0 is a valid empty call.  ws: the decoder's workspace, prepared. */
int cp_online_enroll(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows,
                     const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes, void* stream);
/* on an adaptive workspace: the statistics as they are, frozen */
int cp_online_adapt_enroll(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows,
                           const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes, void* stream);
/* on a multi-stream workspace: the folded weights are shared, so there is no stream index */
int cp_online_multi_enroll(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                           const float* windows, int64_t n_windows, const int32_t* slots, int32_t n_classes, double* acc,
                           void* scratch, size_t scratch_bytes, void* stream);
/* on an adaptive multi-stream workspace: the frozen statistics of stream `index` */
int cp_online_multi_adapt_enroll(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                 int32_t index, const float* windows, int64_t n_windows, const int32_t* slots, int32_t n_classes,
                                 double* acc, void* scratch, size_t scratch_bytes, void* stream);
/* acc (64,17) float64, prior (n_classes,16) f32 -> table (n_classes,16) f32 (see Table above); all on the device */
int cp_online_enroll_table(const double* acc, int32_t n_classes, const float* prior, double mix, int32_t min_windows, float* table,
                           void* stream);

/* ---- head fine-tuning: a user's projection and class rows by gradient, behind the shared encoder ---------------------------
 * Calibration moves statistics and enrolment replaces class rows; neither uses a gradient.  Fine-tuning trains what lies
 * behind the encoder -- the projection W (16,512) with its bias b (16) and the class rows E (K,16), 8,208 + 16 K numbers -- with
 * the loss the model was trained with, on the labelled windows of one user's cued recording (windows and labels as for
 * enrolment above).  T is the decoder's compute dtype (f32 or bf16).
 * Tail input.  u_i (512 values in T) is what the decoder's tail multiplies by the projection for labelled window i: the fc7
 * activation (folded forms), or the BN9-normalised fc7 output with the stream's current statistics frozen (adaptive forms;
 * fine-tuning never moves statistics).  The tail-input entries compute it once, through the chain of the enrol entries in
 * chunks of <= 256 windows with the last layer's output kept: out (n_windows,512) in T, 16-byte aligned.  A row's value does
 * not depend on the chunk or call it falls in.
 * Forward.  z_i = W_T u_i + b with W_T the f32 master W rounded to T, multiplied and summed as the tail of a push does;
 * z^_i = z_i / sqrtf(sum z^2) in f32, so training sees the embedding a push will produce bit for bit; E^_c = E_c / |E_c| in
 * f32 as cp_online_set_classes normalises; l_ic = scale (z^_i . E^_c) for c < K <= 64, the dot product summed as a push sums it.
 * Loss.  L = sum_i w_i (-log softmax_c(l_i)[y_i]) with y_i the slot of window i.  balanced: w_i = 1 / (C n_{y_i}) with C the
 * number of slots that have windows and n_c the windows of slot c; otherwise w_i = 1 / N; w_i is held in f32.  A window whose
 * slot lies outside 0..K-1 has w_i = 0.  scale = 1 is the reference's loss (raw cosines, code/models.py:129).
 * Gradients.  g_ic = w_i scale (p_ic - [c = y_i]);  dz^_i = sum_c g_ic E^_c;  dz_i = (dz^_i - z^_i (z^_i . dz^_i)) / |z_i|;
 * dW = sum_i dz_i u_i^T;  db = sum_i dz_i;  dE^_c = sum_i g_ic z^_i;  dE_c = (dE^_c - E^_c (E^_c . dE^_c)) / |E_c|.  dz stays
 * f32 in the dW product (it is not rounded to T) and u enters as stored.  With anchor = lambda >= 0 every tensor theta gets
 * + lambda (theta - theta_0), theta_0 its value at cp_online_finetune_init.  The loss reported is L, without the anchor's
 * lambda / 2 |theta - theta_0|^2.
 * Update.  Adam as torch.optim.Adam states it (beta 0.9 / 0.999, eps 1e-8, bias-corrected, no weight decay, amsgrad off) on
 * the f32 masters W, b, E with f32 moments, evaluated in float64 per element and rounded once each; rates lr (W, b) and
 * lr_rows (E).  A tensor whose flag is not set is not touched, bit for bit.
 * Order.  Rows are cut into chunks of CP_ONLINE_FINETUNE_CHUNK; chunk j's partial gradients (f32, rows in order) and its
 * weighted loss (float64) are one slab; the update sums the slabs in chunk order in float64.  No floating-point atomics: the
 * result of a step depends on the inputs and the chunk constant only, not on the grid, the device or how the steps were cut
 * into calls.
 * A step is two launches (olf_step_kernel, one workgroup per chunk; olf_update_kernel); n_steps steps are enqueued without a
 * host synchronisation.  None of these entries allocates, synchronises or keeps state in the library; each validates on the
 * host and returns CP_ERR_ARG (a short workspace or scratch: CP_ERR_WORKSPACE) before anything is enqueued.  The entries that
 * read or write a workspace's weights take ws_bytes as exactly the form's own workspace size: the forms lay their weights out
 * differently, so a folded entry on an adaptive workspace, or the reverse, is refused. */
#define CP_ONLINE_FINETUNE_CHUNK 64         /* rows per slab */
#define CP_ONLINE_FINETUNE_PROJECTION 1     /* flags of cp_online_finetune_steps: train W and b */
#define CP_ONLINE_FINETUNE_ROWS 2           /* train E */
/* windows (n_windows,12) f32 as a push makes them -> out (n_windows,512) in T.  scratch: cp_online_enroll_scratch_bytes.
 * n_windows == 0 is a valid empty call. */
int cp_online_tail_inputs(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows, void* out,
                          void* scratch, size_t scratch_bytes, void* stream);
int cp_online_adapt_tail_inputs(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* windows, int64_t n_windows,
                                void* out, void* scratch, size_t scratch_bytes, void* stream);
int cp_online_multi_tail_inputs(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                const float* windows, int64_t n_windows, void* out, void* scratch, size_t scratch_bytes,
                                void* stream);
int cp_online_multi_adapt_tail_inputs(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                      int32_t index, const float* windows, int64_t n_windows, void* out, void* scratch,
                                      size_t scratch_bytes, void* stream);
/* bytes of the caller-owned state (256-byte aligned device memory) of a run over n_windows labelled windows */
size_t cp_online_finetune_state_bytes(int64_t n_windows, int32_t n_classes);
/* W (16,512), b (16), E (n_classes,16) f32 and slots (n_windows) int32 on the device -> masters, theta_0, zero moments, step 0,
 * W_T in `dtype`, and the weights w_i.  One launch. */
int cp_online_finetune_init(void* state, size_t state_bytes, int32_t dtype, const float* W, const float* b, const float* E,
                            const int32_t* slots, int64_t n_windows, int32_t n_classes, int32_t balanced, void* stream);
/* n_steps steps on u (n_windows,512) in T = cfg.dtype, the dtype of the init, 16-byte aligned; n_windows and n_classes as at
 * the init.  loss_out (n_steps) float64 on the device: L of each step, before its update.  n_steps == 0 enqueues nothing. */
int cp_online_finetune_steps(const cp_online_config* cfg, void* state, size_t state_bytes, const void* u, int64_t n_windows,
                             int32_t n_classes, int32_t n_steps, double lr, double lr_rows, double scale, double anchor,
                             int32_t flags, double* loss_out, void* stream);
/* the masters: W (16,512), b (16), E (n_classes,16) f32; grad_out (NULL, or 8208 + 16 n_classes float64): the last step's
 * reduced gradient dW, db, dE with the anchor term.  Device-to-device copies on `stream`. */
int cp_online_finetune_read(void* state, size_t state_bytes, int64_t n_windows, int32_t n_classes, float* W, float* b, float* E,
                            double* grad_out, void* stream);
/* W (16,512), b (16) f32 on the device -> the tail's weights in T and its bias (one launch); and back, widened.  A workspace
 * that never sees a set call is byte for byte what cp_online_*prepare left.  The multi-stream forms share one projection
 * among their streams: it is read, not set (a stream's own goes into a projection bank: "per-stream projections" below). */
int cp_online_set_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* W, const float* b, void* stream);
int cp_online_adapt_set_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* W, const float* b,
                                   void* stream);
int cp_online_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, float* W, float* b, void* stream);
int cp_online_adapt_projection(const cp_online_config* cfg, void* ws, size_t ws_bytes, float* W, float* b, void* stream);
int cp_online_multi_projection(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes, float* W,
                               float* b, void* stream);
int cp_online_multi_adapt_projection(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                     float* W, float* b, void* stream);

/* ---- grasp command gate: rejection, weighted vote and dwell behind the online decoders --------------------------------------
 * A decoder forces every window onto one of its K class rows.  The gate is a stage behind it that reads the logits a push emits
 * (cosines in [-1, 1]) and keeps one state machine per stream, so that the stream can answer "none of these", report how sure
 * it is, hold a grasp through a few ambiguous windows and ask that a new grasp win for some time before the hand moves.  One
 * launch per push for any n_streams <= 256 (one wave per stream, lane k = class slot k); the decoders' own kernels and outputs
 * do not change.  The state lives in a workspace of the gate's own: per stream K, ids[64], min_cosine[64], ring slots [256] and
 * ring weights [256], head and len, the command (a class id, or none), the pending slot and the run length.  A zeroed
 * workspace is a valid start (no classes, empty ring, command none).  cfg.vote is the same on every call of a workspace.
 * Per window, in window order, all float arithmetic in f32 without contraction:
 *   row        k1 = first maximum of the row's K logits, c1 = l[k1], c2 = the maximum over k != k1 (K = 1: -1.0f),
 *              margin = c1 - c2.  A row with a non-finite logit is rejected with conf = margin = NaN; any other row is
 *              accepted iff c1 >= min_cosine[k1] and margin >= min_margin.
 *   ring       the entry (k1 if accepted else -1, w) enters the ring; the oldest leaves once `vote` entries are in.  w = 1
 *              (weight 0, count) or 1 + (int32) rint(min(margin, 2) * 2^20) (weight 1, margin; round-half-even, the product
 *              is exact).  Weights are integers, a full ring sums below 2^31, and sliding sums are exact in any order.
 *   candidate  the slot with the largest weight sum among the slots with >= min_votes ring entries (ties: the smallest slot);
 *              none if no slot qualifies.
 *   command    candidate == command: nothing is pending (run = 0).  candidate none and release == 0: nothing is pending and
 *              the command stays (never release).  candidate == pending: run += 1.  Otherwise pending = candidate, run = 1.
 *              Then, with something pending and run >= dwell (a grasp) or run >= release (none): command = pending, and
 *              nothing is pending.
 *   outputs    command (class id, or -1 for none), accepted (ids[k1] if accepted else -1), conf = c1, margin.
 * So a stream's outputs depend neither on how its rows are cut into calls nor on the streams that share a launch, and with
 * every gate open (min_cosine -2, min_margin 0, min_votes 1, dwell 1, release 1, count weights, the decoder's vote) command
 * equals the decoder's voted bit for bit.
 * The entries keep no state in the library and validate on the host: a bad argument -- a short workspace included -- returns
 * CP_ERR_ARG with a cp_last_error that names the entry, before anything is enqueued. */
typedef struct cp_online_gate_config {
    int32_t vote;            /* ring length, 1..256 */
    int32_t min_votes;       /* >= 1: ring entries a slot needs to be a candidate */
    int32_t dwell;           /* >= 1: windows in a row a new grasp must win before it becomes the command */
    int32_t release;         /* >= 0: windows in a row of "no candidate" before the command becomes none; 0: never */
    int32_t weight;          /* 0: count, 1: margin */
    float min_margin;        /* >= 0 */
} cp_online_gate_config;
/* bytes of the gate's workspace (256-byte aligned) for n_streams streams; zero it before the first call */
size_t cp_online_gate_workspace_bytes(int32_t n_streams);
/* ids (n_classes) int32 ascending, distinct, >= 0 and min_cosine (n_classes) f32, one threshold per row, both on the HOST (they
 * travel as kernel arguments).  Installs them for stream `index`, empties that stream's ring and pending state, and keeps its
 * command if the command's class id is among the new ids (else the command becomes none). */
int cp_online_gate_set_classes(const cp_online_gate_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                               const int32_t* ids, const float* min_cosine, int32_t n_classes, void* stream);
/* ring, pending state and command of stream `index` (every stream for index -1) to none; classes and thresholds stay */
int cp_online_gate_reset(const cp_online_gate_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream);
/* logits (total_rows, ldl) f32 as a decoder's push emits them (ldl = 64 behind the multi-stream decoders, K behind the single
 * ones); row0, m (n_streams) int32 on the device: stream s owns the rows row0[s] .. row0[s] + m[s] - 1, m[s] <=
 * CP_ONLINE_MAX_WINDOWS, total_rows <= CP_ONLINE_MULTI_MAX_ROWS.  command, accepted (total_rows) int32 and conf, margin
 * (total_rows) f32, which may be NULL, receive the rows' outputs.  A stream with m[s] = 0, without classes, with more classes than
 * ldl, or whose rows do not lie inside 0..total_rows-1 is left untouched (its outputs are not written).  Nothing is enqueued for total_rows = 0. */
int cp_online_gate_push(const cp_online_gate_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const float* logits,
                        int32_t ldl, const int32_t* row0, const int32_t* m, int32_t total_rows, int32_t* command,
                        int32_t* accepted, float* conf, float* margin, void* stream);

/* ---- grasp drive: a proportional level and the electrodes' health per window, behind the decoders and the gate ------------
 * The gate says which grasp; a hand also needs how hard.  The drive is a stage behind the decoders that reads the normalised
 * windows a push emits (the per-channel amplitude) and a class id per window (the gate's command, or a decoder's voted or
 * pred), and keeps one state machine per stream in a workspace of its own: one launch per push for any n_streams <= 256 (one
 * wave per stream).  The decoders' and the gate's kernels and outputs do not change.  A zeroed workspace is a valid start (no
 * profile, every channel good, empty ring, inactive, out 0).  cfg.smooth is the same on every call of a workspace.
 * The profile of a stream (cp_online_drive_set_profile; it survives a reset): ids[K] ascending; rest[12], the resting level
 * of each channel in window units; span[K][12], full effort minus rest (<= 0 or NaN: the channel is not used for that class);
 * weight[K][12] in 0..255; low[12], high[12], the plausible range of a channel (-inf / +inf: open).
 * Per window x[12] with class id g (-1: none), in window order; levels are integers out of CP_ONLINE_DRIVE_ONE; every f32
 * operation is a single one without contraction, the division the correctly rounded one:
 *   health     inside_c = isfinite(x_c) && x_c >= low_c && x_c <= high_c.  A good channel that is not inside, or a bad one that
 *              is, adds 1 to its run counter; otherwise the counter becomes 0.  A counter that reaches bad_after (good -> bad) or
 *              good_after (bad -> good) flips the status and becomes 0.  bad = the 12-bit mask of bad channels after that.
 *   raw        k = the slot of g in ids; g == -1 or not in ids: raw = 0.  Otherwise, over the channels with weight[k][c] > 0,
 *              span[k][c] > 0 and status good: a = fminf(fmaxf((x_c - rest_c) / span[k][c], 0), 1) (NaN -> 0),
 *              q = (int32) rintf(a * 4096), raw = floor(sum w q / sum w), 0 if no channel counts.
 *   smooth     raw enters a ring of the last `smooth` values; s = floor(sum of the ring / entries in it).
 *   hysteresis inactive and s >= on_level: active.  Active and s < off_level: inactive.
 *   slew       target = active ? s : 0; out moves towards target by at most `rise` upwards or `fall` downwards.
 *   outputs    drive = (float) out / 4096.f (exact), active (0 / 1), bad (the mask).
 * So a stream's outputs depend neither on how its rows are cut into calls nor on the streams that share a launch, and with
 * smooth 1, on_level = off_level = 0, rise = fall = 4096 and an open range drive equals raw / 4096 in every window.
 * The entries keep no state in the library and validate on the host: a bad argument -- a short workspace included -- returns
 * CP_ERR_ARG with a cp_last_error that names the entry, before anything is enqueued. */
#define CP_ONLINE_DRIVE_ONE 4096          /* full level */
#define CP_ONLINE_DRIVE_MAX_SMOOTH 256    /* ring length */
typedef struct cp_online_drive_config {
    int32_t smooth;          /* ring length, 1..256 */
    int32_t on_level;        /* 0..4096: an inactive stream becomes active at s >= on_level */
    int32_t off_level;       /* 0..on_level: an active stream becomes inactive at s < off_level */
    int32_t rise;            /* 1..4096: the most `out` grows in one window */
    int32_t fall;            /* 1..4096: the most `out` shrinks in one window */
    int32_t bad_after;       /* 1..65535: windows in a row outside its range before a channel is bad */
    int32_t good_after;      /* 1..65535: windows in a row inside its range before a bad channel is good again */
} cp_online_drive_config;
/* bytes of the drive's workspace (256-byte aligned) for n_streams streams; zero it before the first call */
size_t cp_online_drive_workspace_bytes(int32_t n_streams);
/* ids (n_classes) int32 ascending, distinct, >= 0; rest, low, high (12) f32 (rest finite; low, high not NaN, low <= high);
 * span (n_classes, 12) f32; weight (n_classes, 12) int32 in 0..255: all on the HOST (they travel as kernel arguments).
 * Installs them for stream `index` and restarts that stream (every channel good, empty ring, inactive, out 0). */
int cp_online_drive_set_profile(const cp_online_drive_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                                const int32_t* ids, int32_t n_classes, const float* rest, const float* span,
                                const int32_t* weight, const float* low, const float* high, void* stream);
/* restarts stream `index` (every stream for index -1); the profiles stay */
int cp_online_drive_reset(const cp_online_drive_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream);
/* windows (total_rows, ldw) f32 as a decoder's push emits them (ldw >= 12) and cls (total_rows) int32, a class id or -1 per
 * row; row0, m (n_streams) int32 on the device: stream s owns the rows row0[s] .. row0[s] + m[s] - 1, m[s] <=
 * CP_ONLINE_MAX_WINDOWS, total_rows <= CP_ONLINE_MULTI_MAX_ROWS.  drive (total_rows) f32 and active, bad (total_rows) int32
 * receive the rows' outputs.  A stream with m[s] = 0, without a profile, or whose rows do not lie inside 0..total_rows-1 is
 * left untouched (its outputs are not written).  Nothing is enqueued for total_rows = 0. */
int cp_online_drive_push(const cp_online_drive_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const float* windows,
                         int32_t ldw, const int32_t* cls, const int32_t* row0, const int32_t* m, int32_t total_rows,
                         float* drive, int32_t* active, int32_t* bad, void* stream);

/* ---- gate sweep: many gate settings over one cued recording, scored on the device ------------------------------------------
 * A search over the gate's settings is a set of independent runs of the state machine over the same logits.  The sweep runs
 * n_configs of them in one pair of launches (og_rows_kernel: the part of a row no setting enters, once per row; og_sweep_kernel:
 * one wave per config) and scores each command sequence against the cues, so that only a table of integer counters has to
 * leave the device.
 * - Every config starts from the zero gate state: empty ring, nothing pending, command none.
 * - Config g's command sequence is the one cp_online_gate_push produces for the same rows, config and thresholds
 *   (min_cosine[g], one per class slot), in any cut into calls.  Commands are reported as class slots (-1: none): with a fixed
 *   id list slots and ids are the same information.
 * - expected_slot[j] says what the cue asked for in window j: a class slot 0..n_classes-1, -1 for rest (the hand should do
 *   nothing), -2 (or any other negative value) for a window that is not scored.  scores[g] is, with command[-1] = -1 and a
 *   segment a maximal run of consecutive windows with the same expected >= 0, in this order: n_cue (windows with expected >=
 *   0), n_rest (expected == -1), hit (cue windows with command == expected), wrong (cue windows with command >= 0 and command
 *   != expected), false_active (rest windows with command != -1), switches (windows, the unscored ones included, with command[j]
 *   != command[j-1]), segments, reached (segments with a hit), latency_sum (over reached segments: index of the first hit -
 *   index of the segment's first window), wrong_segments (segments with a wrong window).  score_commands of
 *   contrastiveprosthetics_amd/online.py is the definition.
 * - A config's results do not depend on the other configs in the call.
 * - The host checks n_classes in 1..64 and <= ldl, n_configs in 1..CP_ONLINE_GATE_SWEEP_MAX_CONFIGS, n_rows in 1..2^31-1, the
 *   size of scratch and the pointers (commands may be NULL), and returns CP_ERR_ARG with a cp_last_error that names the entry
 *   before anything is enqueued.
 * - The values inside `configs` lie on the device, where the host cannot check them: the caller does (min_margin finite and
 *   >= 0, weight 0 or 1, thresholds not NaN).  A config with vote outside 1..256, min_votes < 1, dwell < 1 or release < 0 gets
 *   all scores -1 and its row of `commands` is not written; the kernel never indexes with such a value. */
#define CP_ONLINE_GATE_SCORES 10
#define CP_ONLINE_GATE_SWEEP_MAX_CONFIGS 65536
/* bytes of the sweep's scratch (256-byte aligned): 12 per row */
size_t cp_online_gate_sweep_scratch_bytes(int64_t n_rows);
int cp_online_gate_sweep(const float* logits, int32_t ldl, int64_t n_rows, int32_t n_classes,
                         const int32_t* expected_slot,          /* (n_rows) device: slot 0..K-1, -1 rest, -2 ignore */
                         const cp_online_gate_config* configs,  /* (n_configs) device */
                         const float* min_cosine,               /* (n_configs, 64) device */
                         int32_t n_configs, void* scratch, size_t scratch_bytes,
                         int64_t* scores,                       /* (n_configs, CP_ONLINE_GATE_SCORES) device */
                         int32_t* commands,                     /* optional (n_configs, n_rows): slot or -1 */
                         void* stream);

/* ---- grasp sequence decoder: fixed-lag Viterbi behind the logits ------------------------------------------------------------
 * The gate counts hard votes; this stage sums evidence.  Behind any decoder's logits it keeps, per stream, the score of the best
 * path into each of K <= 64 class states (slots 0..K-1) and one "none" state (slot K, reported as -1), with a transition cost
 * between states, and it may decide a few windows late.  One launch per push for any n_streams <= 256 (seq_push_kernel: one wave
 * per stream, lane j = class slot j); the decoders' kernels and outputs do not change.  All values are int32 in units of 2^-20.
 * q(x) = (int32) rint(fminf(fmaxf(x, -2), 2) * 2^20), round-half-even, the product exact: the gate's margin quantisation.
 *   model      ids[K] ascending; thr[k] = q(min_cosine[k]) (min_cosine not NaN); a cost matrix C[i][j], (K+1) x (K+1), entry i -> j
 *              the price of being in j one window after i, clamped into 0..CP_ONLINE_SEQ_MAX_COST (2^28: as good as forbidden)
 *              where it is installed; lag L in 0..63.
 *   state      score[K+1], all 0 at the start; a ring of the last CP_ONLINE_SEQ_RING back-pointer rows (bytes); n, the windows
 *              seen since the last reset (it saturates at 2^30).  A zeroed workspace is a valid start (no classes).
 * Per window, in window order:
 *   emission   a row with a non-finite logit among its K: e[.] = 0 (no evidence).  Otherwise e[k] = q(l[k]) - thr[k]; e[K] = 0.
 *   step       best[j] = max_i (score[i] - C[i][j]); bp[j] = the smallest i that attains it (class slots before none);
 *              new[j] = best[j] + e[j].
 *   renormalise  every entry minus max_j new[j], then every entry below CP_ONLINE_SEQ_FLOOR (-2^29) raised to it: scores lie in
 *              [-2^29, 0], and the step's smallest intermediate is -2^29 - 2^28 - 2^22.
 *   now        the first maximum of score (class slots before none); lead = score[now] - the largest score among the other
 *              states (K + 1 >= 2: there is one).
 *   command    none while n <= L.  Otherwise start at now and follow L back-pointer rows, the newest first: the state of the
 *              best path L windows ago.  L = 0: command = now.
 *   outputs    command and now (class id, or -1 for none), lead.
 * So a stream's outputs and workspace depend neither on how its rows are cut into calls nor on the streams that share a launch;
 * with C = 0, min_cosine = -2 and L = 0, now is the first maximum of q(l[k]); with C = 0 and any L, command[t] = now[t-L]; and
 * the path read from the back-pointers is a maximum-score path.  SequenceReference of contrastiveprosthetics_amd/sequence.py
 * restates this in numpy.
 * The entries keep no state in the library and validate on the host: a bad argument -- a short workspace included -- returns
 * CP_ERR_ARG with a cp_last_error that names the entry, before anything is enqueued. */
#define CP_ONLINE_SEQ_RING 64                 /* back-pointer rows kept: lag <= 63 */
#define CP_ONLINE_SEQ_MAX_COST 268435456      /* 2^28 */
#define CP_ONLINE_SEQ_FLOOR (-536870912)      /* -2^29 */
#define CP_ONLINE_SEQ_SWEEP_MAX_CONFIGS 65536
/* bytes of the stage's workspace (256-byte aligned) for n_streams streams; zero it before the first call */
size_t cp_online_seq_workspace_bytes(int32_t n_streams);
/* ids (n_classes) int32 ascending, distinct, >= 0 and min_cosine (n_classes) f32 on the HOST (they travel as kernel arguments);
 * cost (n_classes + 1, n_classes + 1) int32 on the DEVICE, row and column n_classes the none state.  Installs them with `lag`
 * for stream `index` and restarts that stream (scores 0, empty ring, n = 0). */
int cp_online_seq_set_model(int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, const int32_t* ids, const float* min_cosine,
                            int32_t n_classes, const int32_t* cost, int32_t lag, void* stream);
/* restarts stream `index` (every stream for index -1); the model stays */
int cp_online_seq_reset(int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream);
/* logits, ldl, row0, m and total_rows as cp_online_gate_push takes them, with the same limits.  command (total_rows) int32 and
 * now, lead (total_rows) int32, which may be NULL, receive the rows' outputs.  A stream with m[s] = 0, without a model, with more
 * classes than ldl, or whose rows do not lie inside 0..total_rows-1 is left untouched (its outputs are not written).  Nothing is
 * enqueued for total_rows = 0. */
int cp_online_seq_push(int32_t n_streams, void* ws, size_t ws_bytes, const float* logits, int32_t ldl, const int32_t* row0,
                       const int32_t* m, int32_t total_rows, int32_t* command, int32_t* now, int32_t* lead, void* stream);
/* The sweep: n_configs runs of the stage over one cued recording in one pair of launches (seq_rows_kernel: q(l) of every row and
 * its finite flag, once per row; seq_sweep_kernel: one wave per config, from the zero state), scored as cp_online_gate_sweep
 * scores them: expected_slot, the ten counters, their order and `commands` (slots, -1: none) are those of that entry.
 * - Config g runs model configs[g].model of `costs` (n_models, K+1, K+1) with lag configs[g].lag and the thresholds
 *   min_cosine[g]; its command sequence is the one cp_online_seq_push produces for the same rows, in any cut into calls.
 * - A config's results do not depend on the other configs in the call.
 * - The host checks n_classes in 1..64 and <= ldl, n_configs and n_models in 1..65536, n_rows in 1..2^31-1, the size of scratch
 *   and the pointers (commands may be NULL) before anything is enqueued.  The values inside `configs`, `costs` and `min_cosine`
 *   lie on the device: costs are clamped into 0..2^28 as they are read, thresholds must not be NaN (the caller checks), and a
 *   config with lag outside 0..63 or model outside 0..n_models-1 gets all scores -1 and its row of `commands` is not written;
 *   the kernel never indexes with such a value. */
typedef struct cp_online_seq_config {
    int32_t model;           /* 0..n_models-1 */
    int32_t lag;             /* 0..63 */
} cp_online_seq_config;
/* bytes of the sweep's scratch (256-byte aligned): 256 per row */
size_t cp_online_seq_sweep_scratch_bytes(int64_t n_rows);
int cp_online_seq_sweep(const float* logits, int32_t ldl, int64_t n_rows, int32_t n_classes,
                        const int32_t* expected_slot,           /* (n_rows) device: slot 0..K-1, -1 rest, -2 ignore */
                        const int32_t* costs,                   /* (n_models, K+1, K+1) device */
                        int32_t n_models,
                        const cp_online_seq_config* configs,    /* (n_configs) device */
                        const float* min_cosine,                /* (n_configs, 64) device */
                        int32_t n_configs, void* scratch, size_t scratch_bytes,
                        int64_t* scores,                        /* (n_configs, CP_ONLINE_GATE_SCORES) device */
                        int32_t* commands,                      /* optional (n_configs, n_rows): slot or -1 */
                        void* stream);

/* ---- grasp-set search: many class subsets of one cued recording, scored on the device --------------------------------------
 * Which grasps to keep is a search over subsets of the K class slots, and a subset's score is an independent exact integer
 * walk over the same logits.  The sweep runs n_subsets of them in one pair of launches (os_rows_kernel: a row's slots in
 * descending logit order, once per row; os_sweep_kernel: one wave per subset) and only a table of integer counters leaves the
 * device.  score_subset of contrastiveprosthetics_amd/online.py is the definition.  For the subset S given by the bits of
 * subsets[g] (bit k = slot k):
 * - Kept rows.  Row j is kept if expected_slot[j] is negative or a slot of S.  A row cued for a slot outside S is dropped, as
 *   though it had not been recorded; a kept row with a negative expected_slot, or one >= n_classes, feeds the ring and is not
 *   scored.
 * - Raw prediction of a kept row: the first maximum of its logits over the slots of S in ascending slot order (compared with >,
 *   the lowest slot wins a tie: the rule of the decoders and the gate), or none (-1) if any of the row's n_classes logits is not
 *   finite.
 * - Vote: the decoders' ring from an empty ring.  Every kept row's prediction enters, none included (it takes a place and does
 *   not vote); the oldest entry leaves once `vote` entries are in.  The voted prediction is the slot with the most entries in
 *   the ring, the smallest slot among equals, none if no slot has an entry.  For finite logits that is cp_online_gate_push with
 *   every gate open over the kept rows and the columns of S.
 * - scores[g], in this order: n_cue (kept rows with expected_slot in S), hit (of those, raw prediction == expected_slot),
 *   voted_hit (of those, voted prediction == expected_slot), classes_scored (slots of S with a cue row), worst_class,
 *   worst_hit, worst_n: the slot of S, among those with n_c > 0 cue rows, with the smallest voted recall voted_hit_c / n_c
 *   (fractions compared by cross-multiplication in 64 bits, the smallest slot among equals), its voted_hit_c and its n_c;
 *   -1, 0, 0 if no slot of S has a cue row.  class_hits[g][k], if given, is voted_hit_k for all 64 k (0 outside S).
 * - A subset's results do not depend on the other subsets in the call.
 * - The host checks n_classes in 1..64 and <= ldl, n_subsets in 1..CP_ONLINE_SUBSET_SWEEP_MAX_SUBSETS, vote in
 *   1..CP_ONLINE_MAX_VOTE, n_rows in 1..2^31-1, the size and 16-byte alignment of scratch and the pointers (class_hits may be
 *   NULL), and returns CP_ERR_ARG with a cp_last_error that names the entry before anything is enqueued.  It never allocates
 *   and never synchronises.
 * - `subsets` and `expected_slot` lie on the device, where the host cannot check them, and the kernel checks a value before it
 *   indexes with it: a mask that is 0 or has a bit at or above n_classes gets all seven scores -1 and its row of class_hits
 *   is not written. */
#define CP_ONLINE_SUBSET_SCORES 7
#define CP_ONLINE_SUBSET_SWEEP_MAX_SUBSETS 1048576
/* bytes of the sweep's scratch (256-byte aligned): 64 per row */
size_t cp_online_subset_sweep_scratch_bytes(int64_t n_rows);
int cp_online_subset_sweep(const float* logits, int32_t ldl, int64_t n_rows, int32_t n_classes,
                           const int32_t* expected_slot,   /* (n_rows) device: slot, or negative = kept, unscored */
                           const uint64_t* subsets,        /* (n_subsets) device: bit k = slot k */
                           int32_t n_subsets, int32_t vote, void* scratch, size_t scratch_bytes,
                           int64_t* scores,                /* (n_subsets, CP_ONLINE_SUBSET_SCORES) device */
                           int32_t* class_hits,            /* optional (n_subsets, 64) device */
                           void* stream);

/* ---- electrode map: re-donned and dead electrodes in the online decoders ------------------------------------------------------
 * A decoder's model channel d need not be physical electrode d: a sleeve goes back on rotated, an electrode dies.  A map is
 * src[12] int32 and fill[12] float32 per stream, in caller-owned memory the device reads (device memory, or pinned host
 * memory); the decoder's workspace and the front-end state do not change size or layout.
 * - src[d] is the raw column 0..11 that feeds model channel d, or -1: masked.  src need not be a permutation (a dead electrode
 *   may be replaced by a neighbour).  fill[d] is what a masked channel emits, in normalised units (0 is the training mean); it
 *   is read only where src[d] == -1.
 * - A mapped push.  Model channel d is thread d of the front end: it filters raw column src[d], keeps that filter's state in
 *   its own slots of the stream's state (z[d], ring[d], tmp[d], sq0[d]), normalises with mean_std[d] and mean_std[12 + d] and
 *   writes column d of the windows.  A masked channel runs the same recurrences on input 0, so that unmasking it later is well
 *   defined, and every value it emits is fill[d] exactly.  The map is read once per launch and costs no launch.
 * - The channels are independent, so with src[d] >= 0 for every d a mapped decoder fed raw equals an unmapped decoder fed
 *   raw[:, src] bit for bit, in pred, voted, logits and windows and for any cut into pushes.  Everything behind the front end
 *   (encoder, tail, a gate, a drive and its bad electrodes) sees model channels.
 * - Changing a map in mid-stream leaves a filter transient on the channels that changed, as plugging a cable would: the
 *   filter state of channel d was made by the column it read before.  cp_online_reset clears it.
 * - NULL, NULL is the identity and is what the unmapped entries pass: cp_online_push is cp_online_push_mapped with no map.  The
 *   multi-stream forms take one row per stream, (n_streams,12) each.
 * - The host checks that both pointers are given or neither, their alignment, and that the device can read them; where they
 *   lie in pinned host memory also src in -1..11 and fill finite (CP_ERR_ARG, cp_last_error names the entry).  Device memory
 *   the host cannot read: there the kernel takes src < -1 as masked, src > 11 as 11 and a fill that is not finite as 0. */
int cp_online_push_mapped(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                          const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred, int32_t* voted,
                          float* logits, float* windows, void* stream);
int cp_online_adapt_push_mapped(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                                const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                int32_t* voted, float* logits, float* windows, void* stream);
int cp_online_multi_push_mapped(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                int32_t* voted, float* logits, float* windows, void* stream);
int cp_online_multi_adapt_push_mapped(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                      const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                      const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                      int32_t* voted, float* logits, float* windows, void* stream);
/* cp_online_windows under a map: the windows of a recording in model channels */
int cp_online_windows_mapped(const cp_online_config* cfg, void* state, size_t state_bytes, const float* raw, int64_t n_samples,
                             const float* mean_std, const int32_t* map_src, const float* map_fill, float* windows, void* stream);

/* ---- electrode-map sweep: many maps over one cued recording, scored on the device -------------------------------------------
 * Which map a re-donned sleeve needs is a search, and unlike the gate and subset sweeps every candidate needs the encoder
 * again.  score_channel_maps of contrastiveprosthetics_amd/online.py is the definition: for map g a fresh stream of the
 * decoder (same weights and class table, an empty vote ring, the adaptive forms with their current statistics frozen) gets
 * the map and the whole recording; the sweep reproduces that stream's pred and voted exactly.
 * - rms (n_windows,12) f32 is the recording's un-normalised RMS series: cp_online_windows on a zeroed state with mean 0 and
 *   std 1 ((r - 0) / 1 == r in f32), one pass of the front end for all maps.
 * - Row g n_windows + k is window k under map g: x[d] = src[d] >= 0 ? (rms[k][src[d]] - mean[d]) / std[d] : fill[d], the
 *   front end's expression on the same operands, so the row equals the mapped push's window bit for bit.  The rows run
 *   through the decoder's encoder in chunks of chunk_rows rows (0: a default that fills the chip; at most 65536): the
 *   row-parallel layer kernels of the multi-stream push (the adaptive forms: their frozen chain in pieces of <= 256 rows),
 *   then projection, z / |z|, logits and first-maximum argmax through the tail's own device functions.  A row's values do
 *   not depend on the tile, chunk or call it falls in, so neither do the results depend on chunk_rows.
 * - Then one wave per map walks its n_windows predictions in order through the decoders' vote ring from an empty ring
 *   (cfg.vote entries, the smallest id among equals).
 * - pred, voted (n_maps, n_windows) int32 class ids (voted may be NULL).  scores[g]: rows (windows with expected_slot in
 *   0..K-1), raw_hits (of those, pred == cue), voted_hits (of those, voted == cue).  class_hits[g][k], if given, is the voted
 *   hits of slot k for all 64 k.  expected_slot (n_windows) int32 on the device: the cue's slot in the decoder's ascending id
 *   list; a value outside 0..K-1 is not scored.  n_classes is the K of the decoder's table.
 * - The host checks n_maps in 1..CP_ONLINE_MAP_SWEEP_MAX_MAPS, n_classes in 1..64, n_windows >= 1, n_maps * n_windows < 2^31,
 *   cfg (vote in 1..256), the workspace, the map (as the mapped pushes do), pointers and scratch, and returns CP_ERR_ARG (a
 *   scratch that is too small: CP_ERR_WORKSPACE) before anything is enqueued.  It never allocates and never synchronises.
 *   The decoder's stream state, vote ring and statistics are not touched. */
#define CP_ONLINE_MAP_SCORES 3
#define CP_ONLINE_MAP_SWEEP_MAX_MAPS 65536
/* bytes of the sweep's scratch (256-byte aligned) for n_rows = n_maps * n_windows rows: one chunk's windows and activations */
size_t cp_online_map_sweep_scratch_bytes(int64_t n_rows, int64_t chunk_rows, int32_t dtype, int32_t adaptive);
int cp_online_map_sweep(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* rms, int64_t n_windows,
                        const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps, int32_t n_classes,
                        const int32_t* expected_slot, int64_t chunk_rows, void* scratch, size_t scratch_bytes, int32_t* pred,
                        int32_t* voted, int64_t* scores, int32_t* class_hits, void* stream);
/* on an adaptive workspace: the statistics as they are, frozen */
int cp_online_adapt_map_sweep(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* rms, int64_t n_windows,
                              const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps,
                              int32_t n_classes, const int32_t* expected_slot, int64_t chunk_rows, void* scratch,
                              size_t scratch_bytes, int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits,
                              void* stream);
/* on a multi-stream workspace: the class table of stream `index` */
int cp_online_multi_map_sweep(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                              int32_t index, const float* rms, int64_t n_windows, const float* mean_std, const int32_t* map_src,
                              const float* map_fill, int32_t n_maps, int32_t n_classes, const int32_t* expected_slot,
                              int64_t chunk_rows, void* scratch, size_t scratch_bytes, int32_t* pred, int32_t* voted,
                              int64_t* scores, int32_t* class_hits, void* stream);
/* on an adaptive multi-stream workspace: the class table and frozen statistics of stream `index` */
int cp_online_multi_adapt_map_sweep(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                    int32_t index, const float* rms, int64_t n_windows, const float* mean_std,
                                    const int32_t* map_src, const float* map_fill, int32_t n_maps, int32_t n_classes,
                                    const int32_t* expected_slot, int64_t chunk_rows, void* scratch, size_t scratch_bytes,
                                    int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits, void* stream);

/* ---- cue realignment: the onset and offset of each cued movement, from the sEMG itself ---------------------------------------
 * A person starts a cued movement after the cue and lets go late; the labels the model was trained on had been moved onto
 * the activity seen in the sEMG.  These two entries do that for a user's own cued recording, in front of enrolment, without
 * the model.  realign_reference of contrastiveprosthetics_amd/realign.py is the definition; the device equals it in every
 * integer (csrc/online_realign.cuh).
 * - cp_online_realign_activity: a[k] = sum over the 12 channels of q_d, v = (x_d - base_d) * gain_d in two f32 operations
 *   without contraction, r = rint(v) (ties to even), q_d = 0 unless r > 0 (NaN: 0), 255 if r >= 255, else (int)r; 0..3060.
 *   windows (n_rows, ldw) f32 and activity (n_rows) int32 on the device; base and gain are 12 floats each on the HOST (they
 *   travel as kernel arguments).
 * - cp_online_realign: segments (n_segments, 2) int32 rows [s, e) on the device; with M = n_rows, prev_e the e of the row
 *   before (0 for the first) and next_s the s of the row behind (M for the last), a row that is not 0 <= s < e <= M with
 *   prev_e <= s has status 4: out_segments gets s, e, -1, -1, -1, -1, 4, -1 and nothing else of it is read or written.
 *   Otherwise r0 = max(s - context, prev_e, 0), r1 = min(e + max_lag, max(next_s, e), M) (in a table without bad rows that is
 *   max(s - context, prev_e) and min(e + max_lag, next_s)), L = r1 - r0; L > CP_ONLINE_REALIGN_MAX_REGION: status 3.
 *   With the activity clamped to 0..CP_ONLINE_REALIGN_MAX_ACTIVITY, T its sum over [r0, r1): the pairs (o, f) with
 *   s <= o <= min(s + max_lag, e - min_len), max(o + min_len, e - max_lead) <= f <= r1, n_A = f - o, n_R = L - n_A >= min_rest;
 *   S_A the sum over [o, f), S_R = T - S_A, p = S_A^2 n_R + S_R^2 n_A (< 2^61), q = n_A n_R (< 2^24).  A pair has the
 *   contrast if S_A n_R - S_R n_A >= max(min_contrast q, 1).  The choice is the largest p / q among the pairs with the
 *   contrast (status 0), else among all pairs (status 2), fractions compared as exact 128-bit cross products, equals to the
 *   smaller o, then the smaller f; no pair at all: status 1.
 * - out_expected (M) int32: cue[k] where cue[k] < 0, else -2 (IGNORE); then for a row with status 0 and c = cue[s], over
 *   k in [s, r1): c if o + guard <= k < f - guard; else for k < e: -1 (REST) if k < o - guard or k >= f + guard, else -2;
 *   else -2 if k < f + guard, else cue[k].  The ranges [s, r1) of the rows of a table without bad rows are disjoint.
 * - out_segments (n_segments, 8) int32: s, e, r0, r1, onset, offset, status, cue[s] (onset, offset -1 unless status is 0 or
 *   2); out_sums (n_segments, 2) int64: S_A, S_R of the reported pair, else 0.
 * - Two launches (the default labels; one workgroup per segment), no atomics, no floating point, the same bytes on every run.
 *   The host checks n_rows in 1..2^31-1, n_segments in 1..65536, ldw >= 12, the config (below), pointers and alignment (4
 *   bytes, out_sums 8) and returns CP_ERR_ARG with a cp_last_error that names the entry before anything is enqueued.  Both
 *   entries never allocate and never synchronise. */
#define CP_ONLINE_REALIGN_MAX_ACTIVITY 4095
#define CP_ONLINE_REALIGN_MAX_REGION 4096
typedef struct cp_online_realign_config {
    int32_t max_lag;         /* 0..1024: the onset lies at most this far behind the cue's start, the offset behind its end */
    int32_t max_lead;        /* 0..1024: the offset lies at most this far in front of the cue's end */
    int32_t min_len;         /* >= 1, > 2 guard: windows of a movement */
    int32_t min_rest;        /* >= 1: windows of the region outside the movement */
    int32_t context;         /* 0..2048: windows in front of the cue's start that belong to the region */
    int32_t min_contrast;    /* 0..4095: active mean minus resting mean must reach this (and be positive) */
    int32_t guard;           /* >= 0: windows on either side of onset and offset that are not scored */
} cp_online_realign_config;
int cp_online_realign_activity(const float* windows, int32_t ldw, int64_t n_rows, const float* base, const float* gain,
                               int32_t* activity, void* stream);
int cp_online_realign(const int32_t* activity, const int32_t* cue, int64_t n_rows, const int32_t* segments, int32_t n_segments,
                      const cp_online_realign_config* cfg, int32_t* out_expected, int32_t* out_segments, int64_t* out_sums,
                      void* stream);

/* ---- embeddings out of a push ------------------------------------------------------------------------------------------------
 * The tail of every decoder computes e = z / |z|, sixteen floats per window, and gives out only its cosines against the class
 * rows.  These four entries are the mapped pushes (map_src, map_fill NULL: no map) with one more destination: embeddings
 * (rows,16) f32 on the device, NULL for none, rows in the order and packing of pred.  Row j is the e the tail multiplied
 * with the class rows, so logits[j][k] = sum_d e[j][d] * row[k][d] as sequential f32 multiply-adds from 0 reproduces the
 * logits bit for bit.  Everything else a push returns, launches and keeps is unchanged; the eight entries without
 * `embeddings` are these with NULL. */
int cp_online_push_embed(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                         const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred, int32_t* voted,
                         float* logits, float* windows, float* embeddings, void* stream);
int cp_online_adapt_push_embed(const cp_online_config* cfg, void* ws, size_t ws_bytes, const float* raw, int64_t n_samples,
                               const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                               int32_t* voted, float* logits, float* windows, float* embeddings, void* stream);
int cp_online_multi_push_embed(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                               const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                               const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                               int32_t* voted, float* logits, float* windows, float* embeddings, void* stream);
int cp_online_multi_adapt_push_embed(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                     const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                     const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                     int32_t* voted, float* logits, float* windows, float* embeddings, void* stream);

/* ---- prototype tracking: class rows that follow the user between enrolments -------------------------------------------------
 * A stage behind a decoder, as the gate is, with a workspace of its own (cp_online_track_workspace_bytes; a zeroed one is a
 * valid start: no classes).  One launch per push for up to 256 streams, one wave per stream, lane k = class slot k.
 * track_reference of contrastiveprosthetics_amd/track.py is the definition; the device equals it in every integer and bit
 * (csrc/online_track.cuh).
 * - Per stream: K, ids[K] ascending; anchor[K][16] f32, the enrolled unit rows as cp_online_track_set_rows took them, bit for
 *   bit; row[K][16] f32, the current rows, which start as the anchor; acc[K][16] f64, the tracked direction, which starts as
 *   (double)anchor; n_updates[K], n_refused[K] int64; the decoders' vote ring of cfg.vote slots.
 * - Per window j with embedding e, in window order, every f32 and f64 operation on its own (no contraction):
 *   logits: l[k] = sum_d e[d] * row[k][d], d ascending, from 0.f, multiply then add: the tail's operations.
 *   row: k1 = 0, then every k in ascending order with l[k] > l[k1] becomes k1 (the tail's first maximum; a NaN is never
 *   greater, and nothing is greater than a NaN in slot 0).  c1 = l[k1], c2 = the maximum over k != k1 (-1.0f for K = 1),
 *   margin = c1 - c2.
 *   outputs: pred[j] = ids[k1]; voted[j] from the ring as the decoders compute it (k1 enters, the oldest entry leaves once
 *   cfg.vote are in, the slot with the most entries, the smallest among equals); logits[j][0..K-1] if logits is given.
 *   eligible: rate > 0, every logit finite, c1 >= min_cosine, margin >= min_margin, and with agree k1 == this window's voted slot.
 *   update (eligible windows only), f64: a'[d] = (1 - rate) * acc[k1][d] + rate * (double)e[d]; n2 = sum_d a'[d]^2, d
 *   ascending; cand[d] = (float)(a'[d] / sqrt(n2)); f32: ca = sum_d cand[d] * anchor[k1][d], d ascending.  If n2 is finite and
 *   > 0 and ca >= min_anchor_cosine: acc[k1] = a', row[k1] = cand, n_updates[k1] += 1, updated[j] = ids[k1].  Otherwise
 *   n_refused[k1] += 1 and nothing else changes.  updated[j] = -1 for a refused window and for one that was not eligible.
 *   The new row is first used by window j + 1.
 * - What follows: a stream's outputs depend neither on the cut into pushes nor on the streams that share a launch; with
 *   rate = 0 pred, voted and logits are the decoder's own, bit for bit; with min_anchor_cosine above every cosine no row moves.
 * - cp_online_track_set_rows: ids (n_classes) int32 on the HOST, ascending, distinct, in 0..2^31-2; rows (n_classes,16) f32
 *   on the device, taken as they are (unit rows: the decoder's normalised table).  Installs the anchor and resets the stream's
 *   rows, accumulators, counters and ring.
 * - cp_online_track_reset: index -1 for all streams; what = CP_ONLINE_TRACK_RESET_RING empties the ring,
 *   CP_ONLINE_TRACK_RESET_ROWS also puts rows and accumulators back to the anchor and the counters to 0.
 * - cp_online_track_push: embeddings (total_rows,16) f32, 16-byte aligned, what a *_push_embed entry wrote; row0, m
 *   (n_streams) int32 on the device: stream s owns rows row0[s] .. row0[s] + m[s] - 1, m[s] in 0..256.  pred, voted, updated
 *   (total_rows) int32; logits (total_rows, ldl) f32 or NULL.  A stream without classes, with m[s] = 0 or with rows outside
 *   0..total_rows (or K > ldl with logits) is left untouched.
 * - cp_online_track_rows: the current rows (64,16) f32 and the counters (64) int64 each of one stream, device to device;
 *   any of the three may be NULL.  Slots >= K hold 0.
 * - The host checks the config (vote in 1..256, rate in [0,1), agree 0 or 1, no NaN), n_streams in 1..256, the workspace
 *   (256-byte aligned, large enough), indices, counts, pointers and alignment and returns CP_ERR_ARG with a cp_last_error
 *   that names the entry before anything is enqueued.  The entries never allocate and never synchronise. */
#define CP_ONLINE_TRACK_RESET_RING 0
#define CP_ONLINE_TRACK_RESET_ROWS 1
typedef struct cp_online_track_config {
    int32_t vote;                /* 1..256: length of the vote ring */
    int32_t agree;               /* 1: only a window whose slot is also the voted slot may update */
    double rate;                 /* beta in [0, 1): the share of a window in the tracked direction; 0: nothing ever moves */
    float min_cosine;            /* the top cosine an updating window must reach */
    float min_margin;            /* and its lead over the runner-up */
    float min_anchor_cosine;     /* a row never falls below this cosine to its enrolled row */
    int32_t reserved0;
} cp_online_track_config;
size_t cp_online_track_workspace_bytes(int32_t n_streams);
int cp_online_track_set_rows(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                             const int32_t* ids, const float* rows, int32_t n_classes, void* stream);
int cp_online_track_reset(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                          int32_t what, void* stream);
int cp_online_track_push(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const float* embeddings,
                         const int32_t* row0, const int32_t* m, int32_t total_rows, int32_t* pred, int32_t* voted, float* logits,
                         int32_t ldl, int32_t* updated, void* stream);
int cp_online_track_rows(const cp_online_track_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index,
                         float* rows_out, int64_t* n_updates_out, int64_t* n_refused_out, void* stream);

/* ---- tracker sweep: many tracker settings over one recording's embeddings, scored on the device ------------------------------
 * One wave per setting, each from a fresh tracker on rows (n_classes,16) (anchor = rows, empty ring), through the device
 * function cp_online_track_push walks: setting g's pred, voted and updated sequences are the ones a fresh stream of the
 * stage returns for the same embeddings, as class SLOTS (updated: slot or -1); (n_configs, n_rows) int32 each, optional.
 * - expected_slot (n_rows) int32: the cue's slot, -1 for rest, anything else negative: the row is not scored.  tail_from: the
 *   cue rows are counted from 0 in window order, and those with count >= tail_from are "the last quarter" (the caller sets
 *   tail_from = n_cue - n_cue / 4).
 * - scores (n_configs, CP_ONLINE_TRACK_SCORES) int64, over the scored rows: cue rows; cue rows with pred == cue; with voted
 *   == cue; rows that updated; rows that were refused; rows that updated a slot other than the cue's (any update under
 *   rest); pred hits in the last quarter; voted hits in the last quarter.
 * - configs (n_configs) cp_online_track_config on the device, 8-byte aligned; a setting the stage would refuse (vote, rate)
 *   scores -1 in every counter and its sequences are not written.
 * - The host checks n_classes in 1..64, n_configs in 1..CP_ONLINE_TRACK_SWEEP_MAX_CONFIGS, n_rows in 1..2^31-1, pointers and
 *   alignment (embeddings 16 bytes) and returns CP_ERR_ARG before anything is enqueued. */
#define CP_ONLINE_TRACK_SCORES 8
#define CP_ONLINE_TRACK_SWEEP_MAX_CONFIGS 65536
int cp_online_track_sweep(const float* embeddings, int64_t n_rows, int32_t n_classes, const float* rows, const int32_t* expected_slot,
                          int64_t tail_from, const cp_online_track_config* configs, int32_t n_configs, int64_t* scores,
                          int32_t* pred, int32_t* voted, int32_t* updated, void* stream);

/* ---- held-out enrolment scoring: leave-a-repetition-out over one recording's embeddings ---------------------------------------
 * A plan trains class rows on the windows of some repetitions and scores them on the windows of others, as enrolment with
 * masked labels, a fresh decoder and a push would, from the embeddings alone (csrc/online_holdout.cuh).  holdout_reference of
 * contrastiveprosthetics_amd/holdout.py is the definition; the device equals it in every integer and bit.  Every f32 and f64
 * operation is rounded on its own (no contraction).
 * - The recording: embeddings (n_rows,16) f32; slot (n_rows) int32, the cue's class slot, -1 for rest, anything else (also a
 *   slot >= n_classes): the window trains nothing and is not scored; rep (n_rows) int32, the window's repetition in 0..31,
 *   anything else: the window neither trains nor is evaluated.
 * - cp_online_holdout_sums: sums (n_masks,64,17) f64, the accumulator layout of cp_online_enroll.  sums[u][c][d] starts at 0
 *   and takes one add of (double)embeddings[i][d] per window i in ascending i with slot[i] == c and bit rep[i] of
 *   train_masks[u] set; sums[u][c][16] is the count of those windows.  Slots >= n_classes hold 0.  train_masks (n_masks)
 *   uint32 on the device.
 * - cp_online_holdout_tables: for plan t with S = sums[plans[t].sums_index], slot c: len = (double)sqrtf(sum_d prior[c][d]^2)
 *   in f32, d ascending; sn = sqrt(sum_d S[c][d]^2) in f64; enrolled iff S[c][16] >= min_windows and sn > 0;
 *   rows[t][c][d] = (float)((1 - mix) * (double)prior[c][d] + mix * (len * (S[c][d] / sn))), or prior[c][d] itself if not
 *   enrolled: the row cp_online_enroll_table writes.  unit[t][c][d] = rows[t][c][d] / sqrtf(sum_d rows[t][c][d]^2), f32, d
 *   ascending: the row cp_online_set_classes keeps.  rows, unit (n_plans,n_classes,16) f32; prior (n_classes,16) f32.
 * - cp_online_holdout_score: one wave per plan over the windows with bit rep[i] of plans[t].eval set, in ascending i:
 *   l[k] = sum_d embeddings[i][d] * unit[t][k][d] in f32, d ascending, from 0.f (the tail's operations); the prediction is
 *   none (-1) if any of the n_classes logits is not finite, else the first maximum under `>` (the lowest slot on ties); the
 *   decoders' vote ring of `vote` slots runs from empty over the plan's evaluated windows, a "none" takes a place and does not
 *   vote; the voted slot is the one with the most entries, the smallest among equals, none if no slot has an entry.
 *   scores (n_plans, CP_ONLINE_HOLDOUT_SCORES) int64: evaluated windows with a cue slot (n_cue); of those, windows whose
 *   prediction is the cue (pred_hit); whose vote is the cue (voted_hit); evaluated rest windows (n_rest); training windows,
 *   those with a cue slot and bit rep[i] of plans[t].train set (n_train); slots with at least min_windows of them
 *   (n_enrolled); the slot with the smallest voted recall among slots with cue windows, fractions compared by
 *   cross-multiplication in 64 bits, the smallest slot among equals (worst_class, -1 if none), its hits and its count.
 *   confusion, voted_confusion (n_plans,64,64) int32, optional: cell [cue slot][predicted / voted slot] over the cue windows,
 *   "none" not counted.  pred, voted (n_plans,n_rows) int32, optional: slot, -1 none, -3 for a window the plan does not
 *   evaluate.
 * - cp_online_holdout_logits: logits[i][k] = the l[k] above of window i against unit[assign[i]], k < n_classes; NaN where
 *   assign[i] is outside 0..n_plans-1.  assign (n_rows) int32; logits (n_rows, ldl) f32.
 * - plans (n_plans) cp_online_holdout_plan on the device, 8-byte aligned, checked by the kernels: a plan with mix outside
 *   [0, 1] or NaN, min_windows < 1 or sums_index outside 0..n_masks-1 (cp_online_holdout_score, which is not told n_masks:
 *   0..CP_ONLINE_HOLDOUT_MAX_PLANS-1) scores -1 in every counter, and nothing else of it is written.
 * - The host checks n_classes in 1..64, n_rows in 1..2^31-1, n_masks and n_plans in 1..CP_ONLINE_HOLDOUT_MAX_PLANS, vote in
 *   1..256, ldl >= n_classes, pointers and alignment (embeddings and unit 16 bytes where a wave reads whole rows) and returns
 *   CP_ERR_ARG with a cp_last_error that names the entry before anything is enqueued.  The entries never allocate and never
 *   synchronise. */
#define CP_ONLINE_HOLDOUT_SCORES 9
#define CP_ONLINE_HOLDOUT_MAX_PLANS 4096
#define CP_ONLINE_HOLDOUT_MAX_REPS 32
typedef struct cp_online_holdout_plan {
    uint32_t train;              /* bit r: the windows of repetition r train the rows */
    uint32_t eval;               /* bit r: the windows of repetition r are scored */
    int32_t sums_index;          /* which of the n_masks sums holds this plan's training mask */
    int32_t min_windows;         /* a class with fewer training windows keeps its prior row; at least 1 */
    double mix;                  /* in [0, 1]: the share of the prototype in the row */
} cp_online_holdout_plan;
int cp_online_holdout_sums(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot, const int32_t* rep,
                           const uint32_t* train_masks, int32_t n_masks, double* sums, void* stream);
int cp_online_holdout_tables(const double* sums, int32_t n_masks, int32_t n_classes, const float* prior,
                             const cp_online_holdout_plan* plans, int32_t n_plans, float* rows, float* unit, void* stream);
int cp_online_holdout_score(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot, const int32_t* rep,
                            const float* unit, const cp_online_holdout_plan* plans, int32_t n_plans, int32_t vote, int64_t* scores,
                            int32_t* confusion, int32_t* voted_confusion, int32_t* pred, int32_t* voted, void* stream);
int cp_online_holdout_logits(const float* embeddings, int64_t n_rows, int32_t n_classes, const float* unit, int32_t n_plans,
                             const int32_t* assign, float* logits, int32_t ldl, void* stream);

/* ---- posture prototypes: several class rows per grasp, and the stage that answers with the grasp ---------------------------------
 * A grasp made with the arm down, reaching forward or overhead lands in different places of the 16-d space.  The fit finds up to
 * CP_ONLINE_PROTO_MAX_ROWS rows per class from one cued recording's embeddings; the group stage sits behind a decoder that holds
 * such a table, as the gate does, and turns its row logits into class logits, a class prediction and a class vote
 * (csrc/online_prototypes.cuh).  fit_reference and group_reference of contrastiveprosthetics_amd/prototypes.py are the
 * definitions; the device equals them in every integer and bit.  Every f32 and f64 operation is rounded on its own (no
 * contraction); every dot product is sum_d a[d] * b[d] in f32, d ascending, from 0.f.
 *
 * cp_online_proto_fit, one launch (one wave per class; the classes do not meet):
 * - embeddings (n_rows,16) f32, 16-byte aligned; slot (n_rows) int32 on the device, the cue's class slot, anything outside
 *   0..n_classes-1: the window belongs to no class; use (n_rows) uint8 on the device, optional: 0 keeps a window from training;
 *   rows_per_class (n_classes) int32 in HOST memory, each 1..CP_ONLINE_PROTO_MAX_ROWS, their sum <= 64; iters in
 *   0..CP_ONLINE_PROTO_MAX_ITERS; min_windows >= 1.
 * - The windows of slot c are those with slot[i] == c, use[i] != 0 and all 16 components finite, in ascending i.
 * - centre 0 = (float)(S[d] / |S|), S the float64 sum of the windows in window order, |S| = sqrt(sum_d S[d]^2) in f64, d
 *   ascending: the row cp_online_enroll_table writes for a zero prior at mix = 1.  A slot with fewer than min_windows windows or
 *   |S| = 0 is not fitted: its rows, counts, valid and moved are 0 and assign is -1 for its windows.
 * - centre t = 1..R_c-1 (farthest-first): near(i) starts at -inf and takes every dot product with centres 0..t-1 that is > it;
 *   the window with the smallest near (-0 equals +0), the earliest among equals, is copied bit for bit.
 * - `iters` Lloyd rounds: a window goes to the centre with the largest dot product, the first maximum under `>` from centre 0;
 *   per centre the float64 sum in window order and the count; a centre with count > 0 and |S| > 0 becomes (float)(S / |S|),
 *   otherwise it stays.  moved[c][t] counts the windows whose centre differs from the round before (round 0: every window).
 *   A round that moves nothing leaves a fixed point; the device skips the rounds behind it, which would repeat it.
 * - A final assignment against the final centres gives counts[c][q] and assign[i], the row index within the class; assign is -1
 *   for a window that did not train (no class, use = 0, a non-finite component, a slot that is not fitted).
 *   valid[c][q] = the slot is fitted, q < R_c and counts[c][q] >= min_windows.
 * - rows (n_classes,4,16) f32, counts (n_classes,4) int64, valid (n_classes,4) uint8, moved (n_classes,iters) int64 (may be NULL
 *   with iters = 0), assign (n_rows) int32: every element is written.
 *
 * The group stage.  A stage behind a decoder with a workspace of its own (cp_online_group_workspace_bytes; a zeroed one is a
 * valid start: no stream has groups).  `vote` is the ring length, the decoder's.
 * - cp_online_group_set_groups: row_ids (n_rows) int32 ascending, the ids of the decoder's table rows, and class_of_row
 *   (n_rows) int32, the class id of each, both in HOST memory; the groups are the distinct class ids in ascending order.  The
 *   ring empties.
 * - cp_online_group_reset: index -1 for all streams; the ring empties, the groups stay.
 * - cp_online_group_push, the argument shape of cp_online_gate_push: logits (total_rows, ldl) f32, the decoder's row logits;
 *   stream s owns rows row0[s] .. row0[s] + m[s] - 1 (device int32, m <= 256).  Per window, in window order: the class logit of
 *   group g is the first maximum under `>` of its rows' logits in row order (the f32 maximum), a quiet NaN if one of them is a
 *   NaN; a window with a logit among its n_rows that is not finite predicts nothing (pred = row = -1; its class logits are
 *   written by the rule above, +-inf included); otherwise pred is the group with the largest class logit, the smallest group
 *   among equals (-0 equals +0), and row the id of that group's first maximum.  pred enters the decoders' vote ring, a "none"
 *   takes a place and does not vote; voted is the group with the most entries, the smallest among equals, -1 if none has one.
 *   pred, voted (class ids), row (row id) (total_rows) int32; class_logits (total_rows, ldc) f32, optional, columns
 *   0..n_groups-1.  A stream with m = 0, without groups, with more rows than ldl or more groups than ldc is left untouched.
 *   With one row per class pred, voted and class_logits are the decoder's own bit for bit (finite logits).
 * - The host checks before anything is enqueued and returns CP_ERR_ARG with a cp_last_error that names the entry.  The entries
 *   never allocate and never synchronise. */
#define CP_ONLINE_PROTO_MAX_ROWS 4
#define CP_ONLINE_PROTO_MAX_ITERS 64
int cp_online_proto_fit(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot, const uint8_t* use,
                        const int32_t* rows_per_class, int32_t iters, int32_t min_windows, float* rows, int64_t* counts,
                        uint8_t* valid, int64_t* moved, int32_t* assign, void* stream);
size_t cp_online_group_workspace_bytes(int32_t n_streams);
int cp_online_group_set_groups(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, const int32_t* row_ids,
                               const int32_t* class_of_row, int32_t n_rows, void* stream);
int cp_online_group_reset(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream);
int cp_online_group_push(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, const float* logits, int32_t ldl,
                         const int32_t* row0, const int32_t* m, int32_t total_rows, int32_t* pred, int32_t* voted, int32_t* row,
                         float* class_logits, int32_t ldc, void* stream);

/* ---- user metric: within-class whitening of the embedding, and the stage that decodes in the whitened space ----------------------
 * Every stage above compares a window with a class row by a plain cosine, which weighs all sixteen directions alike.  The pooled
 * within-class scatter of one cued recording, shrunk towards the identity and factored, gives a lower-triangular 16 x 16 matrix A
 * per user; a window e becomes A e / |A e| and is compared with class rows fitted in that space (csrc/online_metric.cuh).
 * fit_reference, apply_reference and stage_reference of contrastiveprosthetics_amd/metric.py are the definitions; the device
 * equals them in every integer and bit (the payload of a NaN is not compared).  Every f32 and f64 operation is rounded on its own
 * (no fused multiply-add).
 *
 * cp_online_metric_moments, one launch (one wave per class):
 * - embeddings (n_rows, 16) f32, 16-byte aligned; slot (n_rows) int32, the class slot of each window, anything outside
 *   0..n_classes-1: the window belongs to no class; use (n_rows) uint8, optional: 0: the window does not train.  A class's
 *   windows are those with its slot, use set and 16 finite components, in window order.
 * - counts (n_classes) int64: the windows of each class.  moments (n_classes, CP_ONLINE_METRIC_MOMENTS) f64: S[d], d = 0..15, the
 *   sum of (double)e[d], then P[i][j] for i <= j in i-major order (136 entries), the sum of (double)e[i] * (double)e[j]; every
 *   accumulator starts from 0 and takes one add per window in window order (the product of two f32 values is exact in f64).
 *
 * cp_online_metric_factor, one launch (one wave per shrink value):
 * - shrinks (n_shrinks <= CP_ONLINE_METRIC_MAX_SHRINKS) f64 in host memory, each within [0, 1], checked before the launch.
 * - A class is fitted when counts[c] >= min_windows; C the fitted classes, N their windows.  N - C < 1: no metric.  Else for
 *   i <= j, over the fitted classes in slot order: t = S_c[i] * S_c[j]; t = t / (double)n_c; Sw[i][j] += P_c[i][j] - t; then
 *   Sw[i][j] /= (double)(N - C).  tr = the diagonal summed in order, s = tr / 16; no metric unless s is finite and > 0.
 * - Per shrink value l: B[i][j] = (1 - l) * (Sw[i][j] / s) + (i == j ? l : 0.0).  Cholesky B = L L^T in f64, row by row:
 *   r = B[i][j]; r = r - L[i][k] * L[j][k] for k = 0..j-1; a pivot (i == j) that is not > 0 or not finite: no metric for this
 *   l; L[i][i] = sqrt(r), L[i][j] = r / L[j][j].  The inverse, column j by column j: Ai[j][j] = 1.0 / L[j][j]; for i > j: r = 0.0;
 *   r = r - L[i][k] * Ai[k][j] for k = j..i-1; Ai[i][j] = r / L[i][i].  A = (float)Ai, lower triangular, the rest +0; an entry
 *   that is not finite in f32: no metric for this l.  l = 1 gives the identity in every bit.
 * - A (n_shrinks, 16, 16) f32 and valid (n_shrinks) uint8; where there is no metric valid = 0 and A is the identity, so every
 *   element is written.
 *
 * cp_online_metric_apply, row-parallel over n_rows windows with one A (16, 16) f32 (only its lower triangle is read):
 * - y[i] = the f32 sum over j = 0..i, in that order, from 0, of A[i][j] * e[j]; ss = the f32 sum over i of y[i] * y[i];
 *   out[i] = y[i] / sqrtf(ss).  A window with a component that is not finite, or with y = 0, gives a row that is not finite.
 *
 * The stage.  A stage behind a decoder with a workspace of its own (cp_online_metric_workspace_bytes; a zeroed one is a valid
 * start: no metric, no rows, empty ring), which reads the embeddings of a push (cp_online_*_push_embed).  The entries take ws_bytes
 * as exactly cp_online_metric_workspace_bytes(n_streams).
 * - cp_online_metric_set: A (16, 16) f32 on the device, or NULL: the stream's metric stays; rows (n_classes, 16) f32 on the
 *   device with ids (n_classes) int32 ascending in host memory, or NULL: the stream's rows stay.  The rows are normalised as
 *   cp_online_set_classes normalises a table.  The ring empties.
 * - cp_online_metric_reset: index -1 for all streams; CP_ONLINE_METRIC_RESET_RING empties the ring, CP_ONLINE_METRIC_RESET_ALL
 *   also removes the metric and the rows.
 * - cp_online_metric_push, the argument shape of cp_online_track_push: per window, in window order, e' as cp_online_metric_apply
 *   forms it; logit of slot k = the f32 sum over d = 0..15 of e'[d] * row[k][d]; if a logit of the K slots is not finite the
 *   window predicts nothing (-1), else the first maximum under `>` (-0 equals +0); pred enters the decoders' vote ring, where a
 *   "none" takes a place and does not vote; voted is the slot with the most entries, the smallest among equals, -1 if none has
 *   one.  pred, voted (total_rows) int32 class ids; logits (total_rows, ldl) f32, optional, columns 0..K-1.  A stream with
 *   m = 0, without a metric, without rows, with more rows than ldl, or whose row0 / m leave total_rows is left untouched.
 * - The host checks before anything is enqueued and returns CP_ERR_ARG with a cp_last_error that names the entry.  The entries
 *   never allocate and never synchronise. */
#define CP_ONLINE_METRIC_MOMENTS 152
#define CP_ONLINE_METRIC_MAX_SHRINKS 64
#define CP_ONLINE_METRIC_RESET_RING 0
#define CP_ONLINE_METRIC_RESET_ALL 1
int cp_online_metric_moments(const float* embeddings, int64_t n_rows, int32_t n_classes, const int32_t* slot, const uint8_t* use,
                             double* moments, int64_t* counts, void* stream);
int cp_online_metric_factor(const double* moments, const int64_t* counts, int32_t n_classes, int32_t min_windows,
                            const double* shrinks, int32_t n_shrinks, float* A, uint8_t* valid, void* stream);
int cp_online_metric_apply(const float* embeddings, int64_t n_rows, const float* A, float* out, void* stream);
size_t cp_online_metric_workspace_bytes(int32_t n_streams);
int cp_online_metric_set(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, const float* A,
                         const float* rows, const int32_t* ids, int32_t n_classes, void* stream);
int cp_online_metric_reset(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, int32_t what, void* stream);
int cp_online_metric_push(int32_t vote, int32_t n_streams, void* ws, size_t ws_bytes, const float* embeddings, const int32_t* row0,
                          const int32_t* m, int32_t total_rows, int32_t* pred, int32_t* voted, float* logits, int32_t ldl,
                          void* stream);

/* ---- closed-form head fit: a user's projection by ridge regression onto the unit class rows, without a gradient -------------------
 * The projection (16 x 512 + 16) of a user is fitted in closed form from the tail inputs u (cp_online_*tail_inputs) of a cued
 * recording: x = [u, 1] (CP_ONLINE_READOUT_X = 513 values), targets the unit class rows E^ (n_classes, 16) f32 exactly as
 * cp_online_set_classes normalises them.  fit_reference and apply_reference of contrastiveprosthetics_amd/readout.py are the
 * definitions; moments and solve equal them in every bit, the apply equals the embeddings of a push with the projection installed
 * (cp_online_*set_projection) in every bit.  Every f64 operation is rounded on its own (no fused multiply-add), no atomics.
 *
 * cp_online_readout_moments (two launches: the index lists, then a grid of (tiles, groups)):
 * - u (n_rows, 512) in dtype (CP_F32 or CP_BF16; widened exactly), 16-byte aligned; slot (n_rows) int32, outside 0..n_classes-1:
 *   the window is not used; group (n_rows) int32, outside 0..n_groups-1: not used (n_groups <= CP_ONLINE_READOUT_MAX_GROUPS);
 *   weight (n_rows) f64, the caller's w_i.  All on the device.
 * - Per group r, over its used windows in window order, every element from 0: G[r][a][b] += w_i * (x_ia * x_ib) and
 *   C[r][a][d] += w_i * (x_ia * E^[slot_i][d]): the inner product of two f32 values is exact in f64, then one rounded multiply
 *   by w_i and one rounded add.  G (n_groups, 513, 513) f64, symmetric in every bit, and C (n_groups, 513, 16) f64 are written
 *   whole: an empty group gives zeros, and n_rows == 0 is a valid call.  Windows are staged CP_ONLINE_READOUT_STAGE at a time.
 *
 * cp_online_readout_solve (one launch, one workgroup per plan):
 * - masks (n_plans) uint32 and ridges (n_plans) f64 in host memory, n_plans <= CP_ONLINE_READOUT_MAX_PLANS: plan t trains on the
 *   groups whose bit is set and penalises with ridges[t] >= 0.  n_plans == 0 is a valid empty call.
 * - A = the sum of G[r] over the mask in ascending r, from 0, + ridges[t] on the diagonal entries 0..511 (the bias is not
 *   penalised); B = the sum of C[r] likewise.  Cholesky A = L L^T: element (i, j) starts from A[i][j] and has L[i][k] * L[j][k]
 *   subtracted for k = 0..j-1 in ascending k, one rounded multiply and one rounded subtract each, then sqrt (i == j) or the
 *   division by L[j][j].  A pivot that is not finite or not > 0 at column j: status[t] = j + 1, W[t] and b[t] zero.  Else
 *   status[t] = 0, forward substitution (k ascending), backward substitution (k = a+1.. ascending), for the 16 right-hand sides;
 *   W[t][d][a] = (float)X[a][d], b[t][d] = (float)X[512][d].  W (n_plans, 16, 512), b (n_plans, 16) f32, status (n_plans) int32.
 *
 * cp_online_readout_apply (two launches): u (n_rows, 512) in dtype, W (n_plans, 16, 512) and b (n_plans, 16) f32 on the device;
 *   W is rounded to dtype as cp_online_*set_projection rounds it, z = W u + b is multiplied and summed by the push tail's own
 *   tile code, out[t][i] = z / sqrtf(sum z^2) in f32: (n_plans, n_rows, 16) f32.  n_rows == 0 and n_plans == 0 are valid.
 *
 * scratch: 256-byte aligned, at least cp_online_readout_scratch_bytes(n_rows, n_groups, n_plans) bytes (the largest need of the
 * three entries; an entry ignores the argument it does not take); nothing is kept in it between calls.  The host checks before
 * anything is enqueued and returns CP_ERR_ARG or CP_ERR_WORKSPACE with a cp_last_error that names the entry.  The entries never
 * allocate, never synchronise and keep no state. */
#define CP_ONLINE_READOUT_MAX_GROUPS 16
#define CP_ONLINE_READOUT_MAX_PLANS 256
#define CP_ONLINE_READOUT_STAGE 16
#define CP_ONLINE_READOUT_X 513
size_t cp_online_readout_scratch_bytes(int64_t n_rows, int32_t n_groups, int32_t n_plans);
int cp_online_readout_moments(const void* u, int32_t dtype, int64_t n_rows, const int32_t* slot, const int32_t* group,
                              const double* weight, const float* targets, int32_t n_classes, int32_t n_groups, double* G, double* C,
                              void* scratch, size_t scratch_bytes, void* stream);
int cp_online_readout_solve(const double* G, const double* C, int32_t n_groups, const uint32_t* masks, const double* ridges,
                            int32_t n_plans, float* W, float* b, int32_t* status, void* scratch, size_t scratch_bytes, void* stream);
int cp_online_readout_apply(const void* u, int32_t dtype, int64_t n_rows, const float* W, const float* b, int32_t n_plans, float* out,
                            void* scratch, size_t scratch_bytes, void* stream);

/* ---- per-stream projections: each stream of the multi-stream decoders with a projection of its own ---------------------------
 * The workspace of the multi-stream forms holds one projection for all streams (cp_online_multi*_projection reads it).  A
 * projection bank gives every stream a slot for a user's own (head fine-tuning, closed-form head fit): a device buffer of the
 * caller's, 256-byte aligned, separate from the workspace (whose size and layout do not change), of
 *   cp_online_projections_bytes(n_streams, dtype) = n_streams * (16 * 512 * sizeof(T) + 256) bytes, T = float or bf16.
 * Slot s starts s * (16 * 512 * sizeof(T) + 256) bytes in: W (16,512) in T, rounded exactly as cp_online_*set_projection rounds
 * it; the 16 f32 biases; one "set" word.  A zeroed bank holds no projection (zero it once after allocating).  A stream whose
 * slot is not set decodes with the workspace's projection, and the choice is made on the device: cp_online_multi*_prepare
 * (a refresh) needs no bank call, a user's projection survives it, and an unset stream's outputs are in every bit those of the
 * entries without a bank.  A set stream's outputs are in every bit those of a single-stream decoder of the same form with the
 * same W, b installed (cp_online_*set_projection).
 *
 * - set: W (16,512), b (16) f32 on the device into slot `index` (one launch); get: the slot widened into W, b, and is_set (NULL,
 *   or one int32 on the device: 1 if the slot is set, else 0; an unset slot's W and b are whatever the bank holds); clear: the
 *   set word of slot `index`, or of every slot (index == -1), to zero (one launch).
 * - cp_online_multi_push_proj / cp_online_multi_adapt_push_proj: cp_online_multi_push_embed / cp_online_multi_adapt_push_embed
 *   with `bank`, `bank_bytes` (the bank of the same n_streams and cfg.dtype); workgroup s of the tail launch takes slot s.  The
 *   launches per push do not change.  bank == NULL is the _push_embed entry, launch for launch.
 * - cp_online_multi_enroll_proj / cp_online_multi_adapt_enroll_proj: cp_online_multi_enroll / cp_online_multi_adapt_enroll for
 *   stream `index` with its slot: the accumulated directions are those of the projection the stream decodes with.
 * - cp_online_multi_map_sweep_proj / cp_online_multi_adapt_map_sweep_proj: cp_online_multi_map_sweep /
 *   cp_online_multi_adapt_map_sweep (the push's own tail) for stream `index` with its slot.
 *   In both pairs bank == NULL is the entry they are named after.  cp_online_*tail_inputs are upstream of the projection and
 *   take no bank.
 *
 * The host checks before anything is enqueued: CP_ERR_ARG (a NULL bank where one is required, a misaligned one, dtype, n_streams
 * outside 1..256, a stream index outside 0..n_streams-1) or CP_ERR_WORKSPACE (bank_bytes too small), with a cp_last_error that
 * names the entry.  The entries never allocate, never synchronise and keep no state. */
size_t cp_online_projections_bytes(int32_t n_streams, int32_t dtype);
int cp_online_projections_set(int32_t dtype, void* bank, size_t bank_bytes, int32_t n_streams, int32_t index, const float* W,
                              const float* b, void* stream);
int cp_online_projections_get(int32_t dtype, const void* bank, size_t bank_bytes, int32_t n_streams, int32_t index, float* W, float* b,
                              int32_t* is_set, void* stream);
int cp_online_projections_clear(int32_t dtype, void* bank, size_t bank_bytes, int32_t n_streams, int32_t index, void* stream);
int cp_online_multi_push_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                              const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                              const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred, int32_t* voted,
                              float* logits, float* windows, float* embeddings, const void* bank, size_t bank_bytes, void* stream);
int cp_online_multi_adapt_push_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                    const float* raw, const int32_t* counts, int64_t total_samples, int32_t total_windows,
                                    const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t* pred,
                                    int32_t* voted, float* logits, float* windows, float* embeddings, const void* bank,
                                    size_t bank_bytes, void* stream);
int cp_online_multi_enroll_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                int32_t index, const void* bank, size_t bank_bytes, const float* windows, int64_t n_windows,
                                const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes, void* stream);
int cp_online_multi_adapt_enroll_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                      int32_t index, const void* bank, size_t bank_bytes, const float* windows, int64_t n_windows,
                                      const int32_t* slots, int32_t n_classes, double* acc, void* scratch, size_t scratch_bytes,
                                      void* stream);
int cp_online_multi_map_sweep_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                   int32_t index, const void* bank, size_t bank_bytes, const float* rms, int64_t n_windows,
                                   const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps,
                                   int32_t n_classes, const int32_t* expected_slot, int64_t chunk_rows, void* scratch,
                                   size_t scratch_bytes, int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits,
                                   void* stream);
int cp_online_multi_adapt_map_sweep_proj(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, void* ws, size_t ws_bytes,
                                         int32_t index, const void* bank, size_t bank_bytes, const float* rms, int64_t n_windows,
                                         const float* mean_std, const int32_t* map_src, const float* map_fill, int32_t n_maps,
                                         int32_t n_classes, const int32_t* expected_slot, int64_t chunk_rows, void* scratch,
                                         size_t scratch_bytes, int32_t* pred, int32_t* voted, int64_t* scores, int32_t* class_hits,
                                         void* stream);

/* ---- joint-angle decoding: a ridge pose readout behind the decoders -----------------------------------------------------------
 * Everything above emits a class, or one level beside a class.  This stage emits a pose: per 10 ms window and stream the angle of
 * up to CP_ONLINE_KIN_MAX_JOINTS joints, regressed linearly from the tail inputs (fc7's output, 512 values per window) onto the
 * glove samples recorded alongside the sEMG, then bounded, smoothed and rate-limited by an integer state machine.  The numpy
 * definitions are in contrastiveprosthetics_amd/kinematics.py (window_targets, moments_reference, fit_reference, pose_reference,
 * JointReference, score_reference); every entry equals them in every bit.  Nothing a push launches or emits changes.
 *
 * cp_online_tail_offset (host only): the byte offset, inside the workspace of the form (adaptive, multi) with this config,
 *   n_streams and max_rows (the single-stream forms: n_streams 1, max_rows ignored, cfg->max_windows rows), of the block that
 *   holds the tail inputs of the last push: row r is (512) values in the compute dtype with leading dimension 512 and belongs
 *   to row r of that push's logits (packed (stream, window) in the multi forms).  It stays valid until the next call that runs
 *   the encoder on that workspace.  0 with cp_last_error set for a bad config.
 *
 * cp_online_kin_moments (two launches: the index lists, then a grid of (tiles, groups)): cp_online_readout_moments with the
 *   window's own target row y[i] (n_joints of ldy f32 values) in place of a class row.  u (n_rows, 512) in dtype, 16-byte
 *   aligned; group (n_rows) int32, outside 0..n_groups-1: not used; weight (n_rows) f64.  G (n_groups, 513, 513) f64 and C
 *   (2, n_groups, 513, 16) f64: column block k holds joints 16 k .. 16 k + 15 (joints from n_joints on: zero), so C + k *
 *   n_groups * 513 * 16 goes to cp_online_readout_solve as it is.  scratch: cp_online_readout_scratch_bytes(n_rows, n_groups, 1).
 *
 * cp_online_kin_apply (one launch, grid (row chunks, plans)): out[t][i][d] = W[t][d] . u[i] + b[t][d] in the pose matvec's order:
 *   u widened to f32; partial sum l of 64 takes the products W[d][l + 64 j] * u[l + 64 j], j = 0..7 ascending, from +0.0f, each
 *   product rounded, then added and rounded; p[l] = p[l] + p[l + s] for l < s, s = 32, 16, 8, 4, 2, 1; then p[0] + b[d].
 *   W (n_plans, n_joints, 512) 16-byte aligned and b (n_plans, n_joints) f32 on the device; out (n_plans, n_rows, n_joints) f32.
 *
 * cp_online_kin_score (one launch, one wave per plan): per plan t and joint d, over the rows whose group is in test_masks[t]
 *   (host memory, uint32 bit masks of groups 0..15), in row order, in f64 with every operation rounded on its own:
 *   sums[t][d] = n, sum y, sum y^2, sum p, sum p^2, sum y p, sum (p - y)^2 with p = pred[t][i][d], y = y[i][d] widened.
 *
 * The stage (cp_online_kin_workspace_bytes, _set_model, _reset, _push): one state machine per stream in a workspace of its own,
 *   256-byte aligned; zeroed it is a valid start (no model, empty rings, pose 0).  A stream's model is W (n_joints, 512) and b
 *   (n_joints) f32 ON THE DEVICE (16- and 4-byte aligned; one copy launch installs them) and lo, span (finite, span > 0) and rest
 *   (0..4096) per joint from the host.  Installing a model restarts the stream; reset (index, or -1 for every stream) empties the
 *   rings and zeroes the pose, the models stay.
 *   cp_online_kin_push (one launch, one workgroup per stream): stream s takes rows row0[s] .. row0[s] + m[s] - 1 of tail
 *   (total_rows, ldt) in dtype (ldt >= 512, rows 16-byte aligned) and of cls (total_rows) int32 (class ids, < 0: none; cls may
 *   be NULL).  Per row, in row order, per joint d, levels being integers out of CP_ONLINE_KIN_ONE and every f32 operation single:
 *     a = the pose matvec; t = (a - lo) / span; q = (int) rintf(fminf(fmaxf(t, 0), 1) * 4096), a NaN t or a class < 0: q = rest;
 *     q enters the joint's ring of cfg->smooth entries, s = floor(ring sum / entries); out moves towards s by at most cfg->rate.
 *   raw (a), pose (out) and angle (lo + ((float) out / 4096.f) * span) are (total_rows, CP_ONLINE_KIN_MAX_JOINTS) f32, int32, f32;
 *   columns from the stream's n_joints on are zero.  A stream with m[s] == 0, without a model, with m[s] above
 *   CP_ONLINE_MAX_WINDOWS or with rows outside 0..total_rows-1 is left untouched.  row0, m: (n_streams) int32 on the device.
 *
 * The host checks before anything is enqueued: CP_ERR_ARG or CP_ERR_WORKSPACE with a cp_last_error that names the entry.  The
 * entries never allocate, never synchronise and keep no state outside the stage's workspace. */
#define CP_ONLINE_KIN_MAX_JOINTS 32
#define CP_ONLINE_KIN_MAX_SMOOTH 64
#define CP_ONLINE_KIN_ONE 4096
#define CP_ONLINE_KIN_SUMS 7
typedef struct cp_online_kin_config {
    int32_t smooth;                       /* ring length, 1..CP_ONLINE_KIN_MAX_SMOOTH */
    int32_t rate;                         /* largest change of a joint's level per window, 1..CP_ONLINE_KIN_ONE */
} cp_online_kin_config;
size_t cp_online_tail_offset(const cp_online_config* cfg, int32_t n_streams, int32_t max_rows, int32_t adaptive, int32_t multi);
int cp_online_kin_moments(const void* u, int32_t dtype, int64_t n_rows, const int32_t* group, const double* weight, const float* y,
                          int32_t ldy, int32_t n_joints, int32_t n_groups, double* G, double* C, void* scratch, size_t scratch_bytes,
                          void* stream);
int cp_online_kin_apply(const void* u, int32_t dtype, int64_t n_rows, const float* W, const float* b, int32_t n_plans,
                        int32_t n_joints, float* out, void* stream);
int cp_online_kin_score(const float* pred, const float* y, int32_t ldy, const int32_t* group, const uint32_t* test_masks,
                        int32_t n_plans, int64_t n_rows, int32_t n_joints, double* sums, void* stream);
size_t cp_online_kin_workspace_bytes(int32_t n_streams);
int cp_online_kin_set_model(const cp_online_kin_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, const float* W,
                            const float* b, int32_t n_joints, const float* lo, const float* span, const int32_t* rest, void* stream);
int cp_online_kin_reset(const cp_online_kin_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream);
int cp_online_kin_push(const cp_online_kin_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const void* tail, int32_t dtype,
                       int32_t ldt, const int32_t* cls, const int32_t* row0, const int32_t* m, int32_t total_rows, float* raw,
                       int32_t* pose, float* angle, void* stream);

/* ---- pose filter: a steady-state Kalman stage behind the joint readout --------------------------------------------------------
 * The joint readout above is filtered joint by joint with a ring mean.  This stage carries a model instead: the state is
 * x = [theta (D), omega (D)] around the resting pose c[d] = lo[d] + ((float) rest[d] / 4096.f) * span[d]; how the joints move
 * together between windows (A, W) is fitted to the glove, how wrong the readout is (Q) to its held-out error, and the Riccati
 * recursion is iterated to a fixed gain K, so that a window costs x' = M x + K o with M = (I - K H) A, H = [I 0], o = a - c.  The
 * numpy definitions are in contrastiveprosthetics_amd/kalman.py (moments_reference, design_reference, FilterReference,
 * sweep_reference), which also state the order of every reduction; every entry equals them in every bit, float64 words
 * included.  Nothing a push launches or emits changes.
 *
 * cp_online_kf_moments (one launch, one workgroup per group): a (the readout's prediction) and y (the target) are (n_rows,
 *   n_joints) f32, group (n_rows) int32 (outside 0..n_groups-1: not used), centre (n_joints) f32 in host memory.  theta_k =
 *   y_k - c, omega_k = theta_k - theta_{k-1}, s_k = [theta_k, omega_k], e_k = a_k - y_k (f32 subtractions).  Index k counts for
 *   group r when windows k-1, k and k+1 all have group r.  Per group, over its counted k in order, in f64 (an exact product and
 *   one rounded add per term): count, G = sum s_k s_k^T, C = sum s_{k+1} s_k^T, S = sum s_{k+1} s_{k+1}^T (each (n_groups, 2D, 2D))
 *   and E = sum e_{k+1} e_{k+1}^T (n_groups, D, D).
 *
 * cp_online_kf_design (one launch per CP_ONLINE_KF_PLANS_PER_LAUNCH plans, one workgroup per plan): per plan (host memory) the
 *   group sums over plan.groups in ascending order divided by n; A from (G + lambda I) A^T = C^T by Cholesky with lambda = lam *
 *   tr(G) / (2D); W = rho * (sym(S - A C^T - C A^T + A G A^T) + 1e-6 * tr(S) / (2D) * I); Q = kappa * (E + 1e-6 * tr(E) / D * I);
 *   P = W, then plan.iters times P- = A P A^T + W, K = P- H^T (H P- H^T + Q)^-1 by Cholesky, P = (I - K H) P- (I - K H)^T + K Q K^T.
 *   M (n_plans, 2D, 2D) and K (n_plans, 2D, D) f32, delta (n_plans) f64 = max|P_T - P_{T-1}| / max|P_T|, status (n_plans) int32:
 *   0, 1 (fewer than 2D + 1 samples), 2 (G + lambda I is not positive definite) or 3 (an innovation matrix is not); with a status
 *   M and K are zero and delta is +inf.  scratch: cp_online_kf_design_bytes(n_plans), 256-byte aligned.
 *
 * cp_online_kf_sweep (one launch, one wave per plan): the filter step over the rows whose group is in test_masks[t] (host
 *   memory), in row order, restarted wherever the row before has another group; sums[t][d] = the seven of cp_online_kin_score on
 *   the filtered pose against y (rows whose filtered pose is NaN skipped) and sum (filtered_k - filtered_{k-1})^2 inside runs.
 *   filtered (n_plans, n_rows, n_joints) f32 or NULL: the filtered pose, NaN on the rows outside the plan's mask.
 *
 * The stage (cp_online_kf_workspace_bytes, _set_model, _reset, _push): as the joint-angle stage, with M (2D, 2D) and K (2D, D)
 *   f32 ON THE DEVICE beside W and b.  Per row: a = the pose matvec (raw, the joint-angle stage's bits); o = a - c; before the
 *   first row whose o is all finite filtered is NaN and that row sets x = [o, 0]; later a row with a non-finite o leaves x as it
 *   is, else x'[i] = sum_j M[i][j] x[j] + sum_j K[i][j] o[j], one accumulator, j ascending from +0.0f, each product rounded, then
 *   added; filtered = x[d] + c[d]; t, q, the rate limit and angle follow the joint-angle stage with smooth = 1.  raw, filtered,
 *   pose, angle are (total_rows, CP_ONLINE_KIN_MAX_JOINTS).  Streams are left untouched as cp_online_kin_push leaves them. */
#define CP_ONLINE_KF_MAX_ITERS 1024
#define CP_ONLINE_KF_PLANS_PER_LAUNCH 128
#define CP_ONLINE_KF_SUMS 8
typedef struct cp_online_kf_plan {
    uint32_t groups;                      /* bit mask of the groups the plan is fitted on */
    int32_t iters;                        /* Riccati iterations, 1..CP_ONLINE_KF_MAX_ITERS */
    double lam;                           /* relative ridge of the trajectory fit, >= 0 */
    double rho;                           /* scale of the process noise, > 0 */
    double kappa;                         /* scale of the measurement noise, > 0 */
} cp_online_kf_plan;
typedef struct cp_online_kf_config {
    int32_t rate;                         /* largest change of a joint's level per window, 1..CP_ONLINE_KIN_ONE */
    int32_t reserved0;
} cp_online_kf_config;
int cp_online_kf_moments(const float* a, const float* y, const int32_t* group, int64_t n_rows, int32_t n_joints, int32_t n_groups,
                         const float* centre, double* G, double* C, double* S, double* E, int32_t* count, void* stream);
size_t cp_online_kf_design_bytes(int32_t n_plans);
int cp_online_kf_design(const double* G, const double* C, const double* S, const double* E, const int32_t* count, int32_t n_joints,
                        int32_t n_groups, const cp_online_kf_plan* plans, int32_t n_plans, float* M, float* K, double* delta,
                        int32_t* status, void* scratch, size_t scratch_bytes, void* stream);
int cp_online_kf_sweep(const float* a, const float* y, const int32_t* group, int64_t n_rows, int32_t n_joints,
                       const uint32_t* test_masks, int32_t n_plans, const float* M, const float* K, const float* centre, double* sums,
                       float* filtered, void* stream);
size_t cp_online_kf_workspace_bytes(int32_t n_streams);
int cp_online_kf_set_model(const cp_online_kf_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, const float* W,
                           const float* b, int32_t n_joints, const float* lo, const float* span, const int32_t* rest, const float* M,
                           const float* K, void* stream);
int cp_online_kf_reset(const cp_online_kf_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, int32_t index, void* stream);
int cp_online_kf_push(const cp_online_kf_config* cfg, int32_t n_streams, void* ws, size_t ws_bytes, const void* tail, int32_t dtype,
                      int32_t ldt, const int32_t* cls, const int32_t* row0, const int32_t* m, int32_t total_rows, float* raw,
                      float* filtered, int32_t* pose, float* angle, void* stream);

#ifdef __cplusplus
}
#endif
#endif
