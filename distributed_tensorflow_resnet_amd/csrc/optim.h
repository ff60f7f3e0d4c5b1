// Optimizer-side declarations (see optim.hip).
#pragma once
#include "kernels.h"

namespace dtr {

// Learning-rate schedule evaluated on the device from global_step: an optional linear
// warm-up, then piecewise-constant steps or a cosine / polynomial decay to `end`.
enum LrDecay : int { LR_PIECEWISE = 0, LR_COSINE = 1, LR_POLY = 2 };
struct LrSchedule {
  float init;            // rate used at step 0 (the hook's begin())
  long long warm_steps;  // linear warm-up length W (0 = none)
  float warm_from, warm_to;   // warm_to: the peak rate of a decay schedule
  int nb;                // number of boundaries (<= 7)
  long long bound[7];
  float val[8];
  // cosine / poly (optim_device.h lr_decay_at): with t = step - 1 in [W, D),
  // q = (D - t) / (D - W), lr = end + (warm_to - end) * F(q), F = sinpi(q / 2)^2 or
  // q^power; exactly `end` from t = D on
  int kind;              // LrDecay
  long long decay_steps; // D > W
  float end, power;
};

void sgd_update_pack(float* master, const float* grad, float* mom, long n, const LrSchedule& s,
                     const long long* gstep, float momentum, float wd, float grad_scale,
                     int use_momentum, const ParamSeg* segs, int nseg, bf16* bf, float* lr_out,
                     int update, hipStream_t st);
// OHWI bf16 weight copies by a tiled transpose of the fp32 master (after the update);
// gstep_inc (optional): global_step += 1 in the same launch.
void ohwi_pack(const float* master, const ParamSeg* segs, const long long* tile0, int nseg,
               long long total_tiles, bf16* bf, long long* gstep_inc, hipStream_t s);
// The fused optimizer of the persistent step (sgd_tiles): per parameter segment, the
// work map of one launch that (optionally) sums the split-K weight-gradient slabs,
// applies SGD-momentum + wd and writes both bf16 copies.
struct OptWork {
  const float* part;       // slabs [splits][K'][taps*cslab] (null: the gradient is in grad)
  long long tile0;         // first workgroup of the segment
  int splits, kslab;       // slab count and rows (output channels, padded) of a slab
  int cslab;               // padded input channels of a slab row (taps*cslab columns)
  int tiled;               // 1: tr (tap*C+ci) x tc (co) tiles; 0: 1024-element chunks
  int tr, tc;              // tile rows / columns (<= 64 each)
};
// blk_seg[b] = the segment of workgroup b; ticket: a zero-initialised int the last
// workgroup resets after its global_step += 1 (every workgroup has read the step); null:
// no global_step increment (a launch updating part of the parameters ahead of the last).
// gin (no slabs): the gradient read as bf16 from gin (the bf16 all-reduce's result; the
// fp32 grad is written from it).  pack: no update -- the gradient (slab sums or grad) is
// only written out, as bf16 to gout (or, gout null, as fp32 to grad): the all-reduce's
// input in one launch instead of a grouped reduce plus a cast.
void sgd_tiles(float* master, float* grad, float* mom, const LrSchedule& s, long long* gstep,
               float momentum, float wd, float grad_scale, int use_momentum,
               const ParamSeg* segs, const OptWork* work, const int* blk_seg, int nblocks,
               bf16* bf, float* lr_out, unsigned* ticket, const bf16* gin, bf16* gout, int pack,
               hipStream_t st);
// LARS (lars.hip): per-tensor trust ratios from a deterministic segmented reduction.
constexpr int LARS_CHUNK = 4096;   // elements of a segment summed by one workgroup
struct LarsSeg {
  long long chunk0;        // first workgroup (chunk) of the segment in lars_norms' grid
  int nchunks;             // ceil(numel / LARS_CHUNK)
  int skip;                // 1: not adapted (trust = 1)
};
// part[b] = (sum w^2, sum g^2) over chunk b (fp64), blk_seg[b] = its segment.  master and
// grad must be 16-byte aligned (the aligned body is read in 16-byte loads).
void lars_norms(const float* master, const float* grad, const ParamSeg* segs,
                const LarsSeg* lsegs, const int* blk_seg, int nblocks, double* part,
                hipStream_t st);
// Per segment: wn = ||w||, gn = |grad_scale| ||g|| from its chunks' partials in chunk
// order; trust = eeta wn / (gn + wd wn + epsilon), or exactly 1 for a skipped segment or
// a zero norm.
void lars_trust(const double* part, const LarsSeg* lsegs, int nseg, float eeta, float wd,
                float epsilon, float grad_scale, float* trust, float* wn, float* gn,
                hipStream_t st);
// sgd_update_pack's update with momentum, at the rate lr * trust[segment].
void lars_update_pack(float* master, const float* grad, float* mom, long n, const LrSchedule& s,
                      const long long* gstep, float momentum, float wd, float grad_scale,
                      const ParamSeg* segs, int nseg, const float* trust, bf16* bf,
                      float* lr_out, hipStream_t st);
// Global gradient-norm clipping (clip.hip).  part[b] = sum of squares of grad[b * CLIP_CHUNK,
// min(n, (b + 1) * CLIP_CHUNK)) in fp64, clip_chunks(n) of them; grad must be 16-byte
// aligned and nothing at or past n is read.
constexpr int CLIP_CHUNK = 4096;   // elements summed by one workgroup
int clip_chunks(long long n);
void grad_sqnorm(const float* grad, long long n, double* part, hipStream_t st);
// out[0] = norm = sqrt(sum of the partials, in chunk order), out[1] = scale: 1 if
// norm <= c, c / norm if norm > c, NaN if the sum is not finite (c > 0, inf allowed).
void clip_scale(const double* part, int nchunks, float c, float* out, hipStream_t st);
// sgd_update_pack's update with the gradient scaled by the device value clip[1].
void sgd_clip_update_pack(float* master, const float* grad, float* mom, long n,
                          const LrSchedule& s, const long long* gstep, float momentum, float wd,
                          const float* clip, int use_momentum, const ParamSeg* segs, int nseg,
                          bf16* bf, float* lr_out, hipStream_t st);
// AdamW (adam.hip) in one launch of sgd_update_pack's shape: m (the momentum buffer) and v
// are the two moments, t = *gstep - *start_step + 1 (both only read), the gradient's scale
// is grad_scale or, clip non-null, the device value clip[1]; wd_seg[nseg] is the decay of
// each segment, applied to the gradient (decoupled = 0: l2) or to the weight at the rate
// lr * wd_seg (decoupled = 1).  adam_out (optional): {lr, alpha, (float)t}.  master, grad,
// m and v must be 16-byte aligned; 0 <= beta < 1 and epsilon > 0.
void adam_update_pack(float* master, const float* grad, float* m, float* v, long n,
                      const LrSchedule& s, const long long* gstep, const long long* start_step,
                      float beta1, float beta2, float epsilon, float grad_scale,
                      const float* clip, int decoupled, const ParamSeg* segs, int nseg,
                      const float* wd_seg, bf16* bf, float* lr_out, float* adam_out,
                      hipStream_t st);
// LAMB (lamb.hip): adamw's direction u = m' k1 / (sqrt(v' k2) + epsilon) (+ wd_seg w,
// decoupled) at the per-segment rate lr * trust, trust = ||w|| / ||u|| -- three launches,
// with ohwi_pack after them.  Arguments mean what adam_update_pack's mean; the chunk table
// (lsegs, blk_seg, nblocks) is LARS's.  lamb_moments_norms updates m and v in place and writes
// part[b] = (sum w^2, sum u^2) over chunk b (fp64); master, grad, m and v 16-byte aligned.
void lamb_moments_norms(const float* master, const float* grad, float* m, float* v,
                        const long long* gstep, const long long* start_step, float beta1,
                        float beta2, float epsilon, float grad_scale, const float* clip,
                        int decoupled, const ParamSeg* segs, const LarsSeg* lsegs,
                        const int* blk_seg, int nblocks, const float* wd_seg, double* part,
                        hipStream_t st);
// Per segment: wn = ||w||, un = ||u|| from its chunks' partials in chunk order; trust =
// wn / un, or exactly 1 for a skipped segment or a norm that is not > 0.
void lamb_trust(const double* part, const LarsSeg* lsegs, int nseg, float* trust, float* wn,
                float* un, hipStream_t st);
// w -= (lr * trust[segment]) * u with u formed again from w and the updated m, v (neither the
// gradient nor the clip slot is read), and the bf16 HWIO copy.  adam_out: {lr, alpha, t}.
void lamb_update_pack(float* master, const float* m, const float* v, long n,
                      const LrSchedule& s, const long long* gstep, const long long* start_step,
                      float beta1, float beta2, float epsilon, int decoupled,
                      const ParamSeg* segs, int nseg, const float* wd_seg, const float* trust,
                      bf16* bf, float* lr_out, float* adam_out, hipStream_t st);
// Lion (lion.hip) in one launch of adam_update_pack's shape: c = beta1 m + (1 - beta1) g',
// w' = (w - lr sign(c)) - (lr wd_seg) w, m' = beta2 m + (1 - beta2) g' with g' the gradient
// scaled by grad_scale or, clip non-null, by the device value clip[1].  m (the momentum
// buffer) is the only state.  master, grad and m must be 16-byte aligned; 0 <= beta < 1.
void lion_update_pack(float* master, const float* grad, float* m, long n, const LrSchedule& s,
                      const long long* gstep, float beta1, float beta2, float grad_scale,
                      const float* clip, const ParamSeg* segs, int nseg, const float* wd_seg,
                      bf16* bf, float* lr_out, hipStream_t st);
// RMSProp in TF 1.12's form (rmsprop.hip) in one launch of adam_update_pack's shape:
// ms' = rho ms + (1 - rho) g'^2, centered: mg' = rho mg + (1 - rho) g',
// mom' = momentum mom + (lr g') / sqrt(ms' [- mg'^2] + epsilon), w' = w - mom', with g' the
// gradient scaled by grad_scale or, clip non-null, by the device value clip[1]; the decay
// wd_seg goes into g' (decoupled = 0: l2) or off the old w at lr wd_seg (decoupled).  mom is
// the momentum buffer; mg is read and written only when centered (it may be null otherwise).
// master, grad, ms, mom (and mg) must be 16-byte aligned; 0 <= rho, momentum < 1; epsilon > 0.
void rmsprop_update_pack(float* master, const float* grad, float* ms, float* mg, float* mom,
                         long n, const LrSchedule& s, const long long* gstep, float rho,
                         float momentum, float epsilon, float grad_scale, const float* clip,
                         int centered, int decoupled, const ParamSeg* segs, int nseg,
                         const float* wd_seg, bf16* bf, float* lr_out, hipStream_t st);
// Weight EMA (ema.hip): shadow -= om * (shadow - master) over n elements, om =
// one_minus_decay, or with warm max(one_minus_decay, 9 / (10 + *gstep)).  gstep is only
// read; master and shadow must be 16-byte aligned.
void ema_update(const float* master, float* shadow, long n, const long long* gstep,
                float one_minus_decay, int warm, hipStream_t st);
void step_increment(long long* gstep, hipStream_t s);
int l2_workspace_floats();
void l2_half_sum(const float* v, long n, float* ws, float* out, hipStream_t s);
void fill_f32(float* p, long n, float a, hipStream_t s);
void cast_f32_bf16(const float* a, bf16* b, long n, hipStream_t s);
void cast_bf16_f32(const bf16* a, float* b, long n, hipStream_t s);

}  // namespace dtr
