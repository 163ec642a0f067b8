/*
 * rover_dagger.h -- C ABI of the fused DAgger distillation of the rover policy into a 31 x 31 depth student (librover_hip.so).
 *
 * The reference's RoverEnvCamera exists for "collecting camera data for Learning By Cheating" (rover_camera_env.py): a
 * privileged teacher drives from the 961-ray height scan, a student learns to drive from the on-board depth image.  At a
 * 31 x 31 camera the image has 961 pixels, the width of the height scan, so the student IS the reference's policy network
 * (rover_policy_default_desc(d, 2, 1): encoder 961 -> 80 -> 60, MLP 64 -> 256 -> 160 -> 128 -> 2, tanh) on a 965-wide row whose scan
 * columns hold depth.  Replaces, per env step of a DAgger loop in torch (Ross et al. 2011; no skrl agent exists for it):
 *
 *     row[:, 0:4]   = nan_to_num(env_row[:, 0:4], nan = 0, posinf = FLT_MAX, neginf = 0)          } rover_dagger_rows,
 *     row[:, 4 + p] = depth_scale * min(d_p, depth_clip),  d_p = depth_clip where the pixel is     } rover_dagger_record
 *                     NaN, +-inf or negative; p row-major over the (height, width) render buffer   }
 *     a*  = teacher(nan_to_num(env_row))         tanh mean, exactly rover_policy_forward            } rover_dagger_act
 *     a_s = student(row)                         exactly rover_policy_forward                       }
 *     u   = uniform from Philox4x32-10 keyed by (seed, global env id, counter)                      }
 *     env action = a* if u < beta else a_s;  label = a* into the memory's action slot               }
 *     L   = (1 / 2B) sum (tanh(z) - a*)^2,  dz = (tanh(z) - a*) (1 - tanh(z)^2) / B                  } rover_dagger_update
 *     clip_grad_norm_ (optional), Adam, the replicas the student's inference reads                   }
 *
 * The reference's slicing quirk is part of the contract (models.py:95): the encoder reads columns [3, 964), the heading plus the
 * first 960 pixels; the last pixel (column 964) is stored and never read.
 *
 * The dataset is the TD3 replay memory as it stands (rover_td3.h "Replay memory"): the observation ring holds student rows, the
 * action slot holds a*, reward and terminated are stored as given and never read by the update.
 *
 * Draws: no new stream.  The mixing draw of row r of a call (g = env_id_offset + r, formed in unsigned arithmetic) is column 0 of
 * the TD3 explorer's random steps (rover_td3_explore.h), reused on purpose as rover_sac_collect.h reuses two streams:
 *     w = word 0 of Philox4x32-10(counter = (g, counter & 0xffffffff, counter >> 32, ROVER_TD3_TAG_RANDOM), key = (seed_lo, seed_hi))
 *     u = ((w >> 9) + 0.5) * 2^-23                      (exact, inside (0, 1))
 * so beta = 1 always takes the teacher and beta = 0 always the student, no draw depends on how the envs are split over ranks, and
 * the specification is td3_explore.random_uniforms as it stands.  The batch's row indices are the TD3 collector's stream (tag
 * 0x54335300, rover_td3_collect.h), bit-comparable with rover_td3_collect_record.  A process that runs a TD3 explorer in RANDOM
 * mode and a DAgger collector under one seed and one counter sees the same uniforms in both; give them different seeds if that
 * matters.
 *
 * Conventions as in rover_td3.h and rover_sac_collect.h: plain C, caller-owned DEVICE buffers, int return codes,
 * rover_last_error(), every call asynchronous on `stream`, no allocation, no host synchronisation, no atomics,
 * -ffp-contract=off; bad arguments are refused without a launch.
 *
 * Numerics and reduction order of the update (bit-reproducible from run to run, every order a function of n alone):
 *   - gather, dense forward, reverse, weight gradients and their chunk combine are rover_td3.h's (the same kernel text under
 *     this trainer's state type): MFMA chains over k in ascending groups of 4, rows cut into fixed chunks of 512, chunk partials
 *     added in chunk order;
 *   - tanh is rover_policy_forward's (the Cephes sequence), so tanh(z) of the update equals the inference output of the same z;
 *   - the loss: per 256-row block a fixed halving tree over the rows' (d_0^2 + d_1^2), then one workgroup adds block partials
 *     t, t + 256, ... in order and a fixed halving tree;
 *   - the gradient norm: 64 fixed chunks of the gradient, threads strided, a halving tree per chunk, the 64 partials added by the
 *     same one-workgroup rule; clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), 1 when grad_norm_clip is 0;
 *   - Adam in torch's single-tensor order on the gradient times that coefficient (the product is written back to `grad`).
 */
#ifndef ROVER_DAGGER_H
#define ROVER_DAGGER_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hyper-parameters of the collector (the first five) and of the update (the rest). */
typedef struct rover_dagger_hparams {
    uint32_t seed_lo, seed_hi;        /* Philox key (42, 0)                                                                  */
    int32_t  env_id_offset;           /* global id of row 0 (RoverEnvCfg.env_id_offset) (0)                                  */
    float    depth_clip;              /* metres; also the value of a pixel that is NaN, +-inf or negative (10.0)             */
    float    depth_scale;             /* (0.1)                                                                               */
    float    lr;                      /* Adam's learning rate (3e-4)                                                         */
    float    beta1, beta2, eps;       /* Adam, torch's defaults (0.9, 0.999, 1e-8)                                           */
    float    grad_norm_clip;          /* clip_grad_norm_'s max_norm; 0 = off (0)                                             */
} rover_dagger_hparams;

/* Device-resident state (caller-allocated, 32 bytes, 8-byte aligned, zero it once before the first call). */
typedef struct rover_dagger_state {
    int32_t steps;                    /* Adam steps taken                                                                    */
    int32_t bad_index;                /* 1 once a sampled row fell outside the filled memory (never reset by the library)    */
    float   loss;                     /* (1 / 2B) sum (tanh(z) - a*)^2 of the last update                                    */
    float   grad_norm;                /* the gradient's 2-norm before clipping                                               */
    float   clip_coef;                /* the coefficient the gradient was multiplied by                                      */
    float   step_size, bc2_sqrt;      /* (float)(lr / (1 - beta1^t)), (float)sqrt(1 - beta2^t)                               */
    float   reserved;
} rover_dagger_state;

int    rover_dagger_default_hparams(rover_dagger_hparams *h);
/* sizeof of the two structs: let a binding check its mirrors. */
size_t rover_dagger_hparams_bytes(void);
size_t rover_dagger_state_bytes(void);

/* Floats of the student's parameter vector (its packed block, padded to 64); 0 if `student` is not
 * rover_policy_default_desc(2, 1) packed by rover_policy_pack. */
size_t rover_dagger_param_floats(const rover_policy_desc *student);
/* Device workspace bytes of rover_dagger_update over up to `max_rows` sampled rows; 0 if max_rows < 1. */
size_t rover_dagger_workspace_bytes(int32_t max_rows);

/* One launch: the student rows of n envs.  Replaces torch's where / minimum / mul / cat over the image and nan_to_num over the
 * env rows.
 *   depth            (n, 961)  the render buffer of rover_camera_render at width = height = 31, row-major (height, width)
 *   env_raw          (n, 965)  the env's raw observation rows
 *   rows_out         (n, 965)  the student rows (a ring slot)
 *   teacher_rows_out (n, 965)  nan_to_num(env_raw), what the teacher reads; may be NULL
 * Each thread owns one 16-byte piece of rows_out; a piece that lies inside the pixel columns of one row is one 16-byte load and
 * one 16-byte store (rows_out + 965 r + 4 + p and depth + 961 r + p have the same phase), the pieces that straddle a row's head
 * go float by float.  When a pointer is not 16-byte aligned every piece goes float by float.  The outputs must not alias the
 * inputs. */
int rover_dagger_rows(const rover_dagger_hparams *h, const float *depth, const float *env_raw, int32_t n, float *rows_out,
                      float *teacher_rows_out, void *stream);

/* Two launches of one kernel (16 rows per 512-thread workgroup, the network part the TD3 collector's device function): the teacher
 * on teacher_rows, then the student on student_rows with the draw and the mix in its epilogue.
 *   label_out   (n, 2)  a*: the memory's action slot
 *   env_act_out (n, 2)  a* where u < beta, else a_s: what env.step takes
 *   student_out (n, 2)  a_s, bit-identical to rover_policy_forward(student, student_rows); may be NULL
 *   source_out  (n)     bytes, 1 where the env received the teacher's action; may be NULL
 * Both networks must be the reference architecture with two tanh outputs (ROVER_ERR_UNSUPPORTED otherwise), their packed buffers
 * as in rover_policy_forward (16-byte aligned, n_copies replicas).  beta must lie in [0, 1]. */
int rover_dagger_act(const rover_policy_desc *teacher, const float *teacher_packed, int32_t teacher_copies,
                     const rover_policy_desc *student, const float *student_packed, int32_t student_copies,
                     const rover_dagger_hparams *h, uint64_t counter, float beta, const float *teacher_rows,
                     const float *student_rows, int32_t n, float *label_out, float *env_act_out, float *student_out,
                     uint8_t *source_out, void *stream);

/* One launch: rover_dagger_rows into the next ring slot plus rover_td3_collect_record's bookkeeping, argument for argument:
 *   rew_out[i] = rew[i], term_out[i] = terminated[i] != 0 for i < n        (rew, terminated, rew_out, term_out: all or none NULL)
 *   *ring_pos_entry = ring_pos_value                                        (one lane; ring_pos_entry may be NULL)
 *   idx_out[i] for i < batch, the TD3 collector's indices under `counter`   (idx_out may be NULL: batch, mem_rows unused then)
 * mem_rows must lie in [1, 2^32] when indices are asked for. */
int rover_dagger_record(const rover_dagger_hparams *h, const float *depth, const float *env_raw, int32_t n, float *ring_slot_out,
                        float *teacher_rows_out, const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out,
                        int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out, int32_t batch, int64_t mem_rows,
                        uint64_t counter, void *stream);

/* One imitation step over n sampled rows idx[0 .. n) of the memory (rover_td3.h's ring and indices; a row outside
 * [0, valid_rows) or with a ring position outside [0, slots) reads row 0 instead and sets bad_index, nothing out of range is
 * followed): gather, the student's forward with caches, the loss head, the backward, the weight gradients into `grad`, the
 * gradient norm, Adam on params / adam_m / adam_v (rover_dagger_param_floats floats each, 16-byte aligned) and the n_copies
 * replicas the student's inference reads (replicas may be NULL).  `labels` is the memory's action buffer (valid_rows x 2).
 * dz_out (n x 2 floats, may be NULL) receives dz.  ws: rover_dagger_workspace_bytes(n) bytes or more, 16-byte aligned. */
int rover_dagger_update(const rover_policy_desc *student, const rover_dagger_hparams *h, float *params, float *grad, float *adam_m,
                        float *adam_v, const float *obs_ring, int32_t slots, int32_t num_envs, const int32_t *ring_pos,
                        const float *labels, const int64_t *idx, int32_t n, int64_t valid_rows, void *ws, size_t ws_bytes,
                        void *state, float *replicas, int32_t n_copies, float *dz_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_DAGGER_H */
