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
//
// Mixup (a second label yb and the row's lam, data.hip): with T(y) the target above,
//   target   t    = lam * T(y) + (1 - lam) * T(yb)
//   row loss      = lse - (1 - eps) * (lam * z[y] + (1 - lam) * z[yb]) - (eps / K) * sum_c z[c]
//   gradient g_c  = (softmax(z)_c - t_c) * grad_scale,
//            t_c  = eps / K + (1 - eps) * (lam * [c == y] + (1 - lam) * [c == yb])   (y == yb too)
//   top-1 / top-k are counted against the dominant label: y if lam >= 0.5, else yb
// A row whose lam == 1.f takes the branch above (wave-uniform) and is bit-for-bit that row.
#pragma once

#include "common.h"

namespace dtr {

struct XentRow {
  float lse;             // logsumexp of the valid classes
  float loss;            // the row's loss (0 at eps == 0 for an out-of-range label, as before)
  float top1, topk;      // 0 / 1 flags (topk is 0 when k == 0)
  float t_miss;          // target of a class that is no label of the row: eps / K
  float w_hit, w_hit_b;  // what the first / the second (mixup) label's class adds to it
  __device__ __forceinline__ float prob(float z) const { return __expf(z - lse); }
  // hit / hit_b: the class is the row's first / second label.  (Sums, not a choice among
  // four targets: the compiler turned that choice into an indexed table in scratch memory.)
  __device__ __forceinline__ float grad(float p, bool hit, bool hit_b, float grad_scale) const {
    const float t = t_miss + (hit ? w_hit : 0.f) + (hit_b ? w_hit_b : 0.f);
    return (p - t) * grad_scale;
  }
};

// `z(j)` is this lane's j-th value, class lane + 64 * j; it is only called for classes
// < `classes`.  VPL > 0: that many values per lane, the loops unroll (register-resident
// rows); VPL == 0: ceil(classes / 64) values, whatever `z` reads them from.  `zy` is
// z[y] (any value when y is out of range), the same in every lane.  `yb`, `zyb`, `lam`:
// the mixup partner's label, its logit and the row's weight of y (lam == 1.f: none).
template <int VPL, class Z>
__device__ __forceinline__ XentRow xent_row(Z z, int lane, int classes, int y, float zy,
                                            float eps, int k, int yb = -1, float zyb = 0.f,
                                            float lam = 1.f) {
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
  r.w_hit = 1.f - eps;
  r.w_hit_b = 0.f;
  const bool mixed = lam != 1.f;   // wave-uniform
  float zt = y_ok ? zy : r.lse;    // the target's logit term
  if (mixed) {
    const bool yb_ok = yb >= 0 && yb < classes;
    r.w_hit = (1.f - eps) * lam;
    r.w_hit_b = (1.f - eps) * (1.f - lam);
    zt = lam * zt + (1.f - lam) * (yb_ok ? zyb : r.lse);
    if (!(lam >= 0.5f)) {   // the dominant label takes the precision counts
      y = yb;
      zy = zyb;
    }
  }
  const bool yd_ok = y >= 0 && y < classes;
  if (eps != 0.f) {   // wave-uniform
    float sz = 0.f;
#pragma unroll
    for (int j = 0; j < nv; ++j)
      if (lane + 64 * j < classes) sz += z(j);
    sz = wave_sum(sz);
    r.loss = r.lse - (1.f - eps) * zt - r.t_miss * sz;
  } else {
    r.loss = r.lse - zt;
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
    r.topk = (yd_ok && finite && above < k) ? 1.f : 0.f;
  }
  return r;
}

}  // namespace dtr
