// Exponential moving average of the trainable weights (tf.train.ExponentialMovingAverage
// over tf.trainable_variables()): one streaming launch behind the step's update,
//   om     = warm ? max(one_minus_decay, 9 / (10 + k)) : one_minus_decay
//   shadow = shadow - om * (shadow - master)
// with k = *gstep as the launch finds it (behind the step's global_step += 1: the number
// of completed steps).  This is TF's  shadow -= (1 - decay) * (shadow - var)  with
// decay = min(decay, (1 + k) / (10 + k)); the warm-up term is 1 - (1 + k) / (10 + k) written
// as 9 / (10 + k), so 1 - decay is never formed by cancellation here -- one_minus_decay
// comes rounded once from fp64 on the host.
// 8 bytes read and 4 written per element, nothing reused: 256-thread workgroups, one
// 16-byte load of each buffer and one 16-byte store per thread and trip of a grid-stride
// loop (at most EMA_MAX_BLOCKS workgroups), the n % 4 last elements as scalars.  gstep is
// only read; no atomics, no LDS.
// Cache policy: the master is read with plain loads (the optimizer wrote it a launch or two
// earlier and the next forward's packs came from it); the shadow, touched once per step and
// never in between, is read and written non-temporally (profiles/ema.md has the A/B against
// plain accesses).
#include "common.h"
#include "optim.h"

namespace dtr {

constexpr int EMA_MAX_BLOCKS = 4096;

__global__ void __launch_bounds__(256)
ema_update_kernel(const float* __restrict__ master, float* __restrict__ shadow, long n,
                  const long long* __restrict__ gstep, float one_minus_decay, int warm) {
  float om = one_minus_decay;
  if (warm) om = fmaxf(om, 9.f / (float)(10 + *gstep));
  const long n4 = n >> 2;
  const f32x4* __restrict__ m4 = reinterpret_cast<const f32x4*>(master);
  f32x4* __restrict__ s4 = reinterpret_cast<f32x4*>(shadow);
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const f32x4 m = m4[i];
    f32x4 s = __builtin_nontemporal_load(s4 + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = s[j] - om * (s[j] - m[j]);
    __builtin_nontemporal_store(s, s4 + i);
  }
  const long t = (n4 << 2) + threadIdx.x;   // the last n % 4 elements: workgroup 0
  if (blockIdx.x == 0 && threadIdx.x < 4 && t < n) shadow[t] = shadow[t] - om * (shadow[t] - master[t]);
}

void ema_update(const float* master, float* shadow, long n, const long long* gstep,
                float one_minus_decay, int warm, hipStream_t st) {
  if (n <= 0) return;
  long blocks = ((n >> 2) + 255) / 256;
  if (blocks > EMA_MAX_BLOCKS) blocks = EMA_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)blocks), dim3(256), 0, st, master, shadow,
                     n, gstep, one_minus_decay, warm);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
