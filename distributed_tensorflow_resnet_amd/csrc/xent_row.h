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
//
// Knowledge distillation (a teacher row t of the same layout, alpha, 1 / tau; Hinton et al.
// 2015): with L_h and t_c the hard loss and target above (smoothing and mixup included),
//   q = softmax(t / tau),  p = softmax(z),  p_tau = softmax(z / tau)
//   row loss      = (1 - alpha) * L_h + alpha * tau^2 * sum_c q_c * (log q_c - log p_tau_c)
//   gradient g_c  = ((1 - alpha) * (p_c - t_c) + alpha * tau * (p_tau_c - q_c)) * grad_scale
//   top-1 / top-k stay counted against the labels
// Two more softmaxes per row, each with its own row max (max(z / tau) is max(z) / tau; the
// teacher's is a second max fold), per-lane sums in class order and the xor-shuffle fold.
// The KL sum takes log q_c - log p_tau_c from the two logsumexps,
//   (t_c / tau - lse_t) - (z_c / tau - lse_s),
// never the log of a probability, and a class whose q_c underflowed to 0 adds exactly 0.
// Only classes < K of either row are read.  A row without a teacher (wave-uniform) takes
// none of this and is bit-for-bit the row above.
//
// AugMix's Jensen-Shannon consistency term (Hendrycks et al. 2020) couples THREE rows, the
// clean view and two AugMix views of one image (rows n, n + B, n + 2B of N = 3B): with
// l_i = z_i - lse(z_i), p_i = exp(l_i), weight w and L_h / t_c the hard loss and target above,
//   log M_c  = logsumexp_i(l_ic) - log 3          (max-shifted over the three views)
//   KL_i     = sum_c p_ic * (l_ic - log M_c)      (a class with p_ic == 0 adds exactly 0)
//   JSD      = (KL_0 + KL_1 + KL_2) / 3
//   triple's loss = L_h(z_0, y) + w * JSD,   reported as 3 x that by the clean row, 0 by the others
//   g_ic     = ([i == 0] * 3 * (p_0c - t_c) + w * p_ic * (l_ic - log M_c - KL_i)) * grad_scale
// (grad_scale is 1 / N, so the clean view's hard term weighs 1 / B.)  log M_c replaces the
// paper's clamp of M to [1e-7, 1]: it is never the log of a probability.  Every row keeps its
// own top-1 / top-k flags against the image's label.  The hard part of each row is xent_row;
// jsd_rows is a second step over the three rows' accessors, shared by every `_jsd` kernel.
#pragma once

#include "common.h"

namespace dtr {

struct XentRow {
  float lse;             // logsumexp of the valid classes
  float mx, lgs;         // its two parts, row max and log of the shifted sum (lse = mx + lgs)
  float loss;            // the row's loss (0 at eps == 0 for an out-of-range label, as before)
  float top1, topk;      // 0 / 1 flags (topk is 0 when k == 0)
  float t_miss;          // target of a class that is no label of the row: eps / K
  float w_hit, w_hit_b;  // what the first / the second (mixup) label's class adds to it
  // distillation (kd false: none of these is read)
  bool kd;               // the row has a teacher (wave-uniform)
  float alpha, inv_tau;  // the soft weight and 1 / tau
  float a_tau;           // alpha * tau, the soft gradient's weight
  float lse_s, lse_t;    // logsumexp of z / tau and of t / tau over the valid classes
  __device__ __forceinline__ float prob(float z) const { return __expf(z - lse); }
  // z, t: the class's student and teacher logit (t any value without a teacher).  hit /
  // hit_b: the class is the row's first / second label.  (Sums, not a choice among four
  // targets: the compiler turned that choice into an indexed table in scratch memory.)
  __device__ __forceinline__ float grad(float z, float t, bool hit, bool hit_b,
                                        float grad_scale) const {
    const float tc = t_miss + (hit ? w_hit : 0.f) + (hit_b ? w_hit_b : 0.f);
    const float hard = prob(z) - tc;
    if (!kd) return hard * grad_scale;
    const float soft = __expf(z * inv_tau - lse_s) - __expf(t * inv_tau - lse_t);
    return ((1.f - alpha) * hard + a_tau * soft) * grad_scale;
  }
  // t_c alone (the JSD heads form p_c themselves)
  __device__ __forceinline__ float target(bool hit, bool hit_b) const {
    return t_miss + (hit ? w_hit : 0.f) + (hit_b ? w_hit_b : 0.f);
  }
};

// `z(j)` is this lane's j-th value, class lane + 64 * j; it is only called for classes
// < `classes`.  VPL > 0: that many values per lane, the loops unroll (register-resident
// rows); VPL == 0: ceil(classes / 64) values, whatever `z` reads them from.  `zy` is
// z[y] (any value when y is out of range), the same in every lane.  `yb`, `zyb`, `lam`:
// the mixup partner's label, its logit and the row's weight of y (lam == 1.f: none).
// `t(j)`: the teacher row through an accessor like `z`, called only when `kd` (the row has
// a teacher; wave-uniform) and only for classes < `classes`; `alpha`, `inv_tau`: the soft
// weight and 1 / tau.
template <int VPL, class Z, class T>
__device__ __forceinline__ XentRow xent_row(Z z, int lane, int classes, int y, float zy,
                                            float eps, int k, int yb, float zyb, float lam,
                                            T t, bool kd, float alpha, float inv_tau) {
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
  r.mx = mx;
  r.lgs = __logf(se);
  r.lse = mx + r.lgs;
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
  r.kd = kd;
  if (kd) {   // wave-uniform
    r.alpha = alpha;
    r.inv_tau = inv_tau;
    r.a_tau = alpha / inv_tau;
    float mt = -INFINITY;
#pragma unroll
    for (int j = 0; j < nv; ++j)
      if (lane + 64 * j < classes) mt = fmaxf(mt, t(j));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mt = fmaxf(mt, __shfl_xor(mt, o, 64));
    const float ms = mx * inv_tau;
    mt *= inv_tau;
    float ss = 0.f, st = 0.f;
#pragma unroll
    for (int j = 0; j < nv; ++j)
      if (lane + 64 * j < classes) {
        ss += __expf(z(j) * inv_tau - ms);
        st += __expf(t(j) * inv_tau - mt);
      }
    ss = wave_sum(ss);
    st = wave_sum(st);
    r.lse_s = ms + __logf(ss);
    r.lse_t = mt + __logf(st);
    float kl = 0.f;
#pragma unroll
    for (int j = 0; j < nv; ++j)
      if (lane + 64 * j < classes) {
        const float lq = t(j) * inv_tau - r.lse_t;
        const float q = __expf(lq);
        if (q > 0.f) kl += q * (lq - (z(j) * inv_tau - r.lse_s));
      }
    kl = wave_sum(kl);
    r.loss = (1.f - alpha) * r.loss + (r.a_tau / inv_tau) * kl;
  }
  return r;
}

// The Jensen-Shannon step over a triple (header comment).  mx[i], lgs[i]: view i's row max
// and the log of its shifted sum.  A log-probability is (z - mx) - lgs, not z - lse: with
// logits of magnitude 100 and more, lse's own rounding (half an ulp of 128 and up) would
// enter every l_ic and, times w, the gradient.
struct JsdRows {
  float mx[3], lgs[3], kl[3], w;
  __device__ __forceinline__ float logp(int i, float z) const {
    return (z - sel(mx, i)) - sel(lgs, i);
  }
  __device__ __forceinline__ float jsd() const { return (kl[0] + kl[1] + kl[2]) * (1.f / 3.f); }
  // log M_c from the class's three logits (NaN only where all three p underflowed to 0 with
  // l = -inf; no caller uses it there)
  __device__ __forceinline__ float log_m(float z0, float z1, float z2) const {
    const float l0 = logp(0, z0), l1 = logp(1, z1), l2 = logp(2, z2);
    const float m = fmaxf(l0, fmaxf(l1, l2));
    return m + __logf(__expf(l0 - m) + __expf(l1 - m) + __expf(l2 - m)) - 1.09861229f;
  }
  // w * p_ic * (l_ic - log M_c - KL_i): view i's soft gradient of a class, before grad_scale
  // (`i` may be a run-time view: a choice among three values, not an indexed read)
  __device__ __forceinline__ float soft(int i, float z, float lm) const {
    const float l = logp(i, z), p = __expf(l);
    return p > 0.f ? w * p * (l - lm - sel(kl, i)) : 0.f;
  }
  static __device__ __forceinline__ float sel(const float (&a)[3], int i) {
    return i == 0 ? a[0] : i == 1 ? a[1] : a[2];
  }
  // view i's whole gradient of a class; `r` is that view's XentRow
  __device__ __forceinline__ float grad(int i, const XentRow& r, float z, float lm, bool hit,
                                        float grad_scale) const {
    const float h = i == 0 ? 3.f * (__expf(logp(0, z)) - r.target(hit, false)) : 0.f;
    return (h + soft(i, z, lm)) * grad_scale;
  }
  // what view i's row reports as its loss
  __device__ __forceinline__ float row_loss(int i, const XentRow& r) const {
    return i == 0 ? 3.f * (r.loss + w * jsd()) : 0.f;
  }
};

// `z0(j)`, `z1(j)`, `z2(j)`: the three views' accessors, as xent_row's `z`; `r0..r2` their
// XentRows.  Per-lane sums in class order, then the xor-shuffle fold, as everywhere here.
template <int VPL, class Z0, class Z1, class Z2>
__device__ __forceinline__ JsdRows jsd_rows(Z0 z0, Z1 z1, Z2 z2, int lane, int classes,
                                            const XentRow& r0, const XentRow& r1,
                                            const XentRow& r2, float w) {
  const int nv = VPL > 0 ? VPL : (classes + 63) >> 6;
  JsdRows t;
  t.mx[0] = r0.mx, t.mx[1] = r1.mx, t.mx[2] = r2.mx;
  t.lgs[0] = r0.lgs, t.lgs[1] = r1.lgs, t.lgs[2] = r2.lgs;
  t.w = w;
  float k0 = 0.f, k1 = 0.f, k2 = 0.f;
#pragma unroll
  for (int j = 0; j < nv; ++j)
    if (lane + 64 * j < classes) {
      const float a = z0(j), b = z1(j), c = z2(j);
      const float lm = t.log_m(a, b, c);
      const float l0 = t.logp(0, a), l1 = t.logp(1, b), l2 = t.logp(2, c);
      const float p0 = __expf(l0), p1 = __expf(l1), p2 = __expf(l2);
      if (p0 > 0.f) k0 += p0 * (l0 - lm);
      if (p1 > 0.f) k1 += p1 * (l1 - lm);
      if (p2 > 0.f) k2 += p2 * (l2 - lm);
    }
  t.kl[0] = wave_sum(k0);
  t.kl[1] = wave_sum(k1);
  t.kl[2] = wave_sum(k2);
  return t;
}

}  // namespace dtr
