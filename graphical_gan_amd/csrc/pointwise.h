// What the pointwise translation units share (pointwise.hip, losses.hip, optim.hip, latent.hip): the block size, the capped
// grid-stride grid and the 16-byte alignment test.
#pragma once
#include "common.h"

namespace ggan {
namespace {

constexpr int kBlock = 256;
inline int grid_for(size_t n, int per_thread = 4) {
    size_t b = cdivz(n, (size_t)kBlock * per_thread);
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;   // 256 CUs x 8 blocks, grid-stride the rest
    return (int)b;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace ggan
