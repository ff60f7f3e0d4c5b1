// On-device input-pipeline declarations (see data.hip).
#pragma once
#include "kernels.h"

namespace dtr {

// Mixup arguments of the input launches (data.hip): the host-made Beta(alpha, alpha) table
// the step's lam is read from, and the side outputs the loss heads take.  A null table: no
// mixup, the launch is the unmixed one.  Workgroup n blends its image with that of batch
// position m = (n + shift) % N; {index, shift} are data/cifar.py mixup_draw(seed, step, N,
// table_len).
// CutMix (cut_thresh > 0): a step whose draw falls under cut_thresh (of 2^24; data/cifar.py
// cutmix_draw) pastes one box of position m's image into this one instead of blending: the
// box size is cut_table[index] (ch << 16 | cw, cutmix_table), mix_lam gets 1 - area / (H * W)
// and the fp32 table is not read.  cut_thresh 0 launches the mixup-only kernels.
struct Mixup {
  const float* table = nullptr;   // [table_len] fp32 in [0, 1]
  int table_len = 0;
  const int* labels = nullptr;    // host-fed launches: the batch's labels [N] (read only)
  int* labels_b = nullptr;        // [N] the partner's label
  float* mix_lam = nullptr;       // [N] the step's lam in every row
  int* mix_log = nullptr;         // optional {index, shift}
  const int* cut_table = nullptr; // [table_len] ch << 16 | cw
  unsigned cut_thresh = 0;        // 0 = never CutMix, 2^24 = always
  int* cut_log = nullptr;         // optional {cut, y0, y1, x0, x1, area, cy, cx} (0s: mixup step)
};

void cifar_augment(const uint8_t* img, bf16* out, int N, int H, int W, int Cpad, int pad,
                   unsigned long long seed, const long long* gstep, int train, int* crop_log,
                   void* zero, long zero_bytes, hipStream_t s,
                   const Mixup& mix = Mixup{});   // zero: optional buffer to clear; mixup: 32x32,
                                                  // Cpad 8 only (std::invalid_argument otherwise)
// cifar_augment on a device-resident split: workgroup n picks record
// resident_index(key_seed, *pos, n, N, records, rank, world, shuffle) (data/cifar.py),
// writes its label into labels_out[n] (and the index into idx_log[n] when given) and
// augments it exactly as cifar_augment does with gstep = pos.  32x32, Cpad 8 only.
void cifar_augment_resident(const uint8_t* records_u8, const int* labels_all, bf16* out,
                            int* labels_out, const long long* pos, int N, int H, int W, int Cpad,
                            long records, int rank, int world, int shuffle,
                            unsigned long long key_seed, int pad, unsigned long long seed,
                            int train, int* crop_log, int* idx_log, void* zero, long zero_bytes,
                            hipStream_t s, const Mixup& mix = Mixup{});   // (mix.labels unused)
// the argument checks of the above (std::invalid_argument), for plan recording
void cifar_augment_resident_check(int N, int H, int W, int Cpad, long records, int rank,
                                  int world, long zero_bytes);
void imagenet_u8_pack(const uint8_t* img, bf16* out, int N, int H, int W,
                      unsigned long long seed, const long long* gstep, int train, void* zero,
                      long zero_bytes, int s2d, hipStream_t s,
                      const Mixup& mix = Mixup{});   // uint8 HWC crops -> bf16 NHWC-8 (s2d: [N][H/2][W/2][16])
// space-to-depth stem: 7x7x3xK fp32 HWIO master -> bf16 [K][4][4][16]; 4x4x16xK fp32
// HWIO gradient -> 7x7x3xK (data.hip)
void stem_s2d_pack(const float* w7, bf16* w4, int K, hipStream_t s);
void stem_s2d_grad(const float* g4, float* g7, int K, hipStream_t s);
void nhwc_pad_channels(const float* x, bf16* out, long npix, int C, int Cpad, hipStream_t s);
void synthetic_images(bf16* out, long npix, int C, int Cpad, unsigned long long seed,
                      hipStream_t s);

}  // namespace dtr
