// The Adam update of ONE parameter, shared by every kernel that applies it to the hash table (optim.hip: the streaming kernels;
// hashgrid_bwd_binned.hip: the slice owners' write-out), so that they agree bit for bit: one expression tree, one set of compiler
// decisions.  Semantics: apex FusedAdam as the reference configures it (/root/reference/train.py:131-137; adam_w_mode = True,
// apex's default: DECOUPLED weight decay, p -= lr * wd * p next to the Adam term; optim.py refuses adam_w_mode=False), bias corrections bc1 = 1 - beta1^t, bc2 = 1 - beta2^t.
#pragma once
#include "ngp_common.h"

struct AdamCoef { float lr, beta1, beta2, eps, wd, bc1, bc2, inv_scale; };

// g_raw: the gradient as stored (loss-scaled); inv_scale undoes the scale
__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g_raw, const AdamCoef& c) {
    const float gk = g_raw * c.inv_scale;
    m = c.beta1 * m + (1.f - c.beta1) * gk;
    v = c.beta2 * v + (1.f - c.beta2) * gk * gk;
    const float denom = sqrtf(v / c.bc2) + c.eps;
    p = p - c.lr * ((m / c.bc1) / denom + c.wd * p);
}

// Dynamic loss scale on the device (torch.cuda.amp.GradScaler's rule, which Lightning's precision=16 puts on top of tiny-cuda-nn's
// fixed 128 in the reference, train.py:274): state = {f32 scale[2], i32 growth_tracker[2]}.  The launches of a step read slot
// `slot` (the field backward multiplies its seeds by scale[slot], the field update divides the gradients by it -- powers of two:
// exact); the first MLP workgroup of the update writes slot ^ 1: scale * backoff and tracker 0 when the step's flag is raised, else
// tracker + 1, and scale * growth every `interval` clean steps.  Readers and the writer never share a word inside a launch.
struct LossScaler { float* state; int slot; float growth, backoff; int interval; float lo, hi; };      // state == NULL: none

// One field update (optim.hip): the grid block and both MLP blocks in one launch, as the ngp_adam_step_field* entry points
// (include/ngp_hip.h) and the native stepper describe it.  The grid gradient is the f16 table, or the dense levels' K partial
// tables summed in the launch (`merge`), or this rank's pieces of every chunk of an exchanged table (`piece` > 0).
struct FieldAdam {
    float* grid_param; ngp_half* grid_param_h; ngp_half* grid_grad; float* grid_m; float* grid_v; int64_t n_grid;
    float* density_param; ngp_half* density_param_h; const float* density_partials; float* density_m; float* density_v; int n_density;
    float* rgb_param; ngp_half* rgb_param_h; const float* rgb_partials; float* rgb_m; float* rgb_v; int n_rgb;
    int n_partials; float lr, beta1, beta2, eps, weight_decay; int step; float grad_scale; int zero_grid_grad;
    const int32_t* found_inf; const int32_t* found_inf_grid; int32_t* step_state;    // skip flags of the MLP / grid blocks, applied-step counts
    const ngp_grid_partials* merge;                                                   // or NULL
    int64_t piece; int32_t n_chunks, world, rank;                                     // piece == 0: the whole table
};
// Validates the record (each gradient source's layout included), builds the device records and launches; 0 or an NGP_E* / HIP code.
__attribute__((visibility("hidden"))) int launch_field_adam(const FieldAdam& f, const LossScaler& scaler, hipStream_t stream);
