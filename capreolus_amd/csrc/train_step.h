// The arithmetic every fused training step shares (capamd_{knrm,drmm,drmmtks,convknrm,pacrr}_train_step): the trainer's pairwise loss
// with its derivative, the mean loss, and torch.optim.Adam's update.  Written once so that the five steps cannot drift apart.
//
// Reference: the loop body of PytorchTrainer.single_train_iteration, capreolus/trainer/pytorch.py:93-108 - self.loss(...) is
// pair_hinge_loss / pair_softmax_loss (reranker/common.py:96-103), self.optimizer.step() the plain torch.optim.Adam (no weight decay,
// no amsgrad).  The update restates Adam's non-capturable single-tensor path (torch/optim/adam.py) op by op: fused-trained checkpoints
// stay interchangeable with the reference trainer's only as long as this order holds.
#pragma once
#include <hip/hip_runtime.h>

namespace capamd {

// The step's scalars, computed by the caller in double from its own step count t (engine.AdamStep.advance):
// step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t).
struct AdamScalars {
  float step_size, one_minus_beta1, beta2, eps, bc2_sqrt;
};

// One element: its parameter p and moments m (exp_avg), v (exp_avg_sq) updated in place from its gradient g.  (`s` by reference: passed
// by value, the five scalars are loaded at the call and the SLP vectorizer may pair the exp_avg update with another add, which unfuses its fma.)
__device__ __forceinline__ void adam_update(float* p, float* m, float* v, float g, const AdamScalars& s) {
  float mm = *m, vv = *v;
  mm = mm + (g - mm) * s.one_minus_beta1;                // exp_avg.lerp_(grad, 1 - beta1)
  vv = vv * s.beta2 + (1.f - s.beta2) * (g * g);         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  *m = mm;
  *v = vv;
  const float denom = sqrtf(vv) / s.bc2_sqrt + s.eps;    // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  *p = *p - s.step_size * (mm / denom);                  // param.addcdiv_(exp_avg, denom, value = -lr / bias_correction1)
}

// One pair's loss (loss_type 0: hinge, 1: softmax of the two scores) and d (mean loss) / d score of its positive and negative document
// (inv_b = 1 / batch).
__device__ __forceinline__ float pair_loss(float s_pos, float s_neg, int loss_type, float inv_b, float& g_pos, float& g_neg) {
  float loss;
  if (loss_type == 0) {
    const float margin = 1.f - (s_pos - s_neg);
    loss = fmaxf(margin, 0.f);
    const float on = margin >= 0.f ? inv_b : 0.f;        // (torch.clamp's backward passes the gradient at the boundary)
    g_pos = -on;
    g_neg = on;
  } else {
    const float mx = fmaxf(s_pos, s_neg), e0 = expf(s_pos - mx), e1 = expf(s_neg - mx), p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
    loss = 1.f - p0;
    g_pos = -p0 * p1 * inv_b;
    g_neg = p0 * p1 * inv_b;
  }
  return loss;
}

// The batch's mean loss from the pairs' losses, summed in pair order by the one thread that calls it.
__device__ __forceinline__ void write_mean_loss(const float* pair_losses, int B, float inv_b, float* loss_out) {
  float l = 0.f;
  for (int i = 0; i < B; ++i) l += pair_losses[i];
  loss_out[0] = l * inv_b;
}

// The entry points' check of the step scalars they share: a known loss type and a positive sqrt(bias_correction2) (NaN fails).
inline bool train_step_scalars_ok(int loss_type, float bc2_sqrt) { return loss_type >= 0 && loss_type <= 1 && bc2_sqrt > 0.f; }

}  // namespace capamd
