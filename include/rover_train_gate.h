/*
 * rover_train_gate.h -- C ABI of the gated PPO update of the rover networks: skrl's KL early stop and its scheduler switch,
 * decided and obeyed on the device (librover_hip.so).
 *
 * skrl 1.1 PPO._update, with rover_ppo.yaml's `kl_threshold: 0.008` and no `learning_rate_scheduler`:
 *
 *     for epoch in range(learning_epochs):
 *         kl_divergences = []
 *         for minibatch in sampled_batches:
 *             states = state_preprocessor(states, train=not epoch)
 *             ... ratio, kl = ((ratio - 1) - log ratio).mean();  kl_divergences.append(kl)
 *             if kl_threshold and kl > kl_threshold: break            # before loss.backward() / optimizer.step()
 *             ... backward, clip_grad_norm_, optimizer.step()
 *         if learning_rate_scheduler: scheduler.step(mean(kl_divergences))
 *
 * A host `if kl > threshold: break` costs one synchronisation per minibatch (240 per update at the reference's shape).  Here
 * the decision is one word of device memory, `rover_ppo_epoch.stop`: the last kernel of a minibatch sets it, every later kernel
 * of the epoch reads it first and returns, and rover_ppo_epoch_end clears it.  The host enqueues the same launches whatever
 * happens and synchronises once, at the end of the update.
 *
 * Rules for the stop word:
 *   - only single-workgroup kernels write it: the last kernel of rover_ppo_minibatch_gated (one workgroup; every thread reads the
 *     word on entry, thread 0 writes it after the workgroup's barriers) and rover_ppo_epoch_end (one thread).  No kernel with
 *     more than one workgroup writes it, so no workgroup ever reads the word in a launch that writes it from another one;
 *   - the order of the launches on the stream is the only synchronisation: no atomics, no fences, no flags between workgroups;
 *   - it is written with ordinary vector stores from plain C++.
 *
 * With `stop` clear every gated entry is bit-identical to its ungated twin in rover_train.h (the same device code, inlined behind
 * one load and a uniform branch); the ungated entries and their kernels are unchanged.  Conventions as in rover_train.h.
 */
#ifndef ROVER_TRAIN_GATE_H
#define ROVER_TRAIN_GATE_H

#include <stddef.h>
#include <stdint.h>

#include "rover_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device-resident state of one epoch (caller-allocated, 32 bytes, 8-byte aligned, zeroed by the caller before the first use). */
typedef struct rover_ppo_epoch {
    int32_t stop;            /* set once a minibatch's KL exceeds the threshold; cleared by rover_ppo_epoch_end              */
    int32_t recorded;        /* minibatch KLs recorded this epoch; cleared by rover_ppo_epoch_end                          */
    int32_t epochs;          /* epochs closed so far                                                                       */
    int32_t stopped_epochs;  /* of those, epochs that stopped early                                                        */
    int32_t stop_minibatch;  /* index of the record that set `stop` in the latest stopped epoch; -1 once an epoch has been */
                             /* closed and none has stopped yet                                                            */
    float stop_kl;           /* that record's KL (0 with stop_minibatch == -1)                                             */
    int32_t reserved[2];
} rover_ppo_epoch;

/* sizeof(rover_ppo_epoch): lets a binding check its mirror of the struct. */
size_t rover_ppo_epoch_bytes(void);

/* rover_ppo_minibatch behind the stop word.  Arguments as rover_ppo_minibatch, then:
 *   kl_early_stop  skrl's kl_threshold (0.008 in rover_ppo.yaml); <= 0: no minibatch ever sets `stop`;
 *   epoch          rover_ppo_epoch (device).
 * epoch->stop set: each of the three kernels returns after reading that one word; grad, stats, mean_out, value_out and the
 * workspace are not written.  Otherwise every output is bit-identical to rover_ppo_minibatch's, then recorded += 1, and if
 * kl_early_stop > 0 and stats[0] > kl_early_stop (strict, fp32: a NaN KL does not stop, as in skrl) stop = 1,
 * stop_minibatch = the index of this record in the epoch and stop_kl = stats[0]. */
int rover_ppo_minibatch_gated(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h,
                              const float *params, const float *obs, const float *act, const float *logp, const float *val,
                              const float *ret, const float *adv, const int64_t *idx, int32_t n, void *ws, size_t ws_bytes,
                              float *grad, float *stats, float *mean_out, float *value_out, float kl_early_stop, void *epoch,
                              void *stream);

/* rover_ppo_apply behind the stop word.  epoch->stop set: nothing is written -- state->step does not move, parameters,
 * moments, replicas, `grad` and the workspace stay as they are (skrl's `break` comes before the offending minibatch's
 * optimizer.step()).  Otherwise bit-identical to rover_ppo_apply. */
int rover_ppo_apply_gated(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h,
                          float *params, float *grad, float *adam_m, float *adam_v, void *state, float *replicas_policy,
                          float *replicas_value, int32_t n_copies, void *ws, size_t ws_bytes, const void *epoch, void *stream);

/* Closes an epoch, one thread on the device.  kl = (sum of stats[4 m], m = 0 .. min(recorded, n_minibatches), in order) /
 * recorded: the mean of the KLs that were recorded, the stopping one included (skrl appends it before the break);
 * recorded == 0: kl = 0 and lr is left alone.  schedule == 1: rover_ppo_kl_schedule's rule on that mean; schedule == 0: lr is
 * not touched (rover_ppo.yaml has no learning_rate_scheduler).  Then epochs += 1, stopped_epochs += stop, stop_minibatch = -1 and
 * stop_kl = 0 while stopped_epochs is still 0, stop = recorded = 0.  kl_out (1 float, may be NULL) receives kl.  `stats`: the
 * n_minibatches consecutive 4-float records of the epoch; records past a stop are not read. */
int rover_ppo_epoch_end(const rover_ppo_hparams *h, const float *stats, int32_t n_minibatches, void *state, void *epoch,
                        int32_t schedule, float *kl_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TRAIN_GATE_H */
