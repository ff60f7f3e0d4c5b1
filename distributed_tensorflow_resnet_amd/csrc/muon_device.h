// What muon.hip and muon_tiled.hip share: the Newton-Schulz coefficients and the momentum
// formulas, one rounding per operation.
#pragma once
#include "optim_device.h"

namespace dtr {

constexpr float NS_A = 3.4445f, NS_B = -4.7750f, NS_C = 2.0315f;

__device__ __forceinline__ void muon_moment(float g, float& m, float s, float mu, int nesterov,
                                            float& u) {
#pragma clang fp contract(off)
  const float gp = s * g;
  const float mm = mu * m;
  m = mm + gp;
  const float t = mu * m;
  u = nesterov ? gp + t : m;
}

}  // namespace dtr
