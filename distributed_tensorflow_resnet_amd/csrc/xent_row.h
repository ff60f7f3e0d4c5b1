// One logits row of the loss head, shared by every row producer (softmax_xent_kernel,
// softmax_xent_rows_kernel, head_fused_kernel and the persistent forward's head) so the
// formulas cannot drift:
//   target   t_c  = (1 - eps) * [c == y] + eps / K        (tf.losses.softmax_cross_entropy
//   row loss      = lse - (1 - eps) * z[y] - (eps / K) * sum_c z[c]    label_smoothing=eps)
//   gradient g_c  = (softmax(z)_c - t_c) * grad_scale
//   top-1         = first argmax == y                       (tf.argmax)
//   top-k         = 0 <= y < K, z[y] finite, #{c < K : z[c] > z[y]} < k   (tf.nn.in_top_k)
// At eps == 0 every value is bit-for-bit the unsmoothed head's: t_c is exactly 1 or 0 and
// the loss takes the `lse - z[y]` branch (wave-uniform).  One wave owns a row; lane l holds
// classes l, l + 64, ...; every sum is per lane in class order, then an xor-shuffle fold.
#pragma once

#include "common.h"

namespace dtr {

struct XentRow {
  float lse;             // logsumexp of the valid classes
  float loss;            // the row's loss (0 at eps == 0 for an out-of-range label, as before)
  float top1, topk;      // 0 / 1 flags (topk is 0 when k == 0)
  float t_hit, t_miss;   // targets of the label's class and of every other class
  __device__ __forceinline__ float prob(float z) const { return __expf(z - lse); }
  __device__ __forceinline__ float grad(float p, bool hit, float grad_scale) const {
    return (p - (hit ? t_hit : t_miss)) * grad_scale;
  }
};

// `z(j)` is this lane's j-th value, class lane + 64 * j; it is only called for classes
// < `classes`.  VPL > 0: that many values per lane, the loops unroll (register-resident
// rows); VPL == 0: ceil(classes / 64) values, whatever `z` reads them from.  `zy` is
// z[y] (any value when y is out of range), the same in every lane.
template <int VPL, class Z>
__device__ __forceinline__ XentRow xent_row(Z z, int lane, int classes, int y, float zy,
                                            float eps, int k) {
  const int nv = VPL > 0 ? VPL : (classes + 63) >> 6;
  XentRow r;
  float mx = -INFINITY;
  int amax = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < nv; ++j) {
    const int c = lane + 64 * j;
    if (c < classes) {
      const float v = z(j);
      if (v > mx) { mx = v; amax = c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {   // first max on ties, like tf.argmax
    const float om = __shfl_xor(mx, o, 64);
    const int oa = __shfl_xor(amax, o, 64);
    if (om > mx || (om == mx && oa < amax)) { mx = om; amax = oa; }
  }
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < nv; ++j)
    if (lane + 64 * j < classes) se += __expf(z(j) - mx);
  se = wave_sum(se);
  r.lse = mx + __logf(se);
  const bool y_ok = y >= 0 && y < classes;
  r.t_miss = eps / (float)classes;
  r.t_hit = (1.f - eps) + r.t_miss;
  if (eps != 0.f) {   // wave-uniform
    float sz = 0.f;
#pragma unroll
    for (int j = 0; j < nv; ++j)
      if (lane + 64 * j < classes) sz += z(j);
    sz = wave_sum(sz);
    r.loss = r.lse - (1.f - eps) * (y_ok ? zy : r.lse) - r.t_miss * sz;
  } else {
    r.loss = r.lse - (y_ok ? zy : r.lse);
  }
  r.top1 = (amax == y) ? 1.f : 0.f;
  r.topk = 0.f;
  if (k > 0) {   // wave-uniform
    int above;
    if (VPL == 1) {   // one class per lane: ballot + popcount
      above = __popcll(__ballot(lane < classes && z(0) > zy));
    } else {
      float n = 0.f;
#pragma unroll
      for (int j = 0; j < nv; ++j)
        if (lane + 64 * j < classes && z(j) > zy) n += 1.f;
      above = (int)wave_sum(n);   // small integers: exact in fp32
    }
    const bool finite = fabsf(zy) < INFINITY;   // false for NaN
    r.topk = (y_ok && finite && above < k) ? 1.f : 0.f;
  }
  return r;
}

}  // namespace dtr
