// ge_rotate_dev.h -- the arithmetic of one complex coordinate of RotatE, shared by ge_rotate.hip (scoring, the hinge step)
// and ge_rotate_adv.hip (the self-adversarial step): the rotation, the difference, its modulus term and dD/du.
#pragma once
#include "ge_common.h"

namespace ge {

constexpr int kRotMaxDim = 1024;

// One complex coordinate of one triple under the rotation (c, s): w = h e^{i theta}, u = w - t, m2 = |u|^2.
struct Coord { float wre, wim, ure, uim, m2; };

__device__ __forceinline__ Coord coord(float hre, float him, float tre, float tim, float c, float s) {
  Coord x;
  x.wre = hre * c - him * s;
  x.wim = hre * s + him * c;
  x.ure = x.wre - tre;
  x.uim = x.wim - tim;
  x.m2 = x.ure * x.ure + x.uim * x.uim;
  return x;
}

// The same coordinate from an already rotated w: u = w - t.
__device__ __forceinline__ Coord coord_rotated(float wre, float wim, float tre, float tim) {
  Coord x;
  x.wre = wre;
  x.wim = wim;
  x.ure = wre - tre;
  x.uim = wim - tim;
  x.m2 = x.ure * x.ure + x.uim * x.uim;
  return x;
}

template <bool L1>
__device__ __forceinline__ float dist_term(const Coord& x) { return L1 ? sqrtf(x.m2) : x.m2; }

// g = dD/du of one coordinate
template <bool L1>
__device__ __forceinline__ void dist_grad(const Coord& x, float& gre, float& gim) {
  if constexpr (L1) {
    const float m = sqrtf(x.m2);
    gre = m > 0.f ? x.ure / m : 0.f;
    gim = m > 0.f ? x.uim / m : 0.f;
  } else {
    gre = 2.f * x.ure;
    gim = 2.f * x.uim;
  }
}

}  // namespace ge
