// kernels_layout.hpp -- device helpers shared by the kernels that move frame-major data into and out of the row layout: the
// transposes of kernels_generic.hpp and the packed-label kernels of kernels_packed.hpp.
#pragma once
#include "kernels_common.hpp"

namespace lutldpc {

// XCD-aware block order of the transposes.  A block moves 128 nodes x one frame group; its frame-major side is one 128-byte
// segment per frame at a stride of N bytes, so unless N is a multiple of 128 every segment straddles two 128-byte lines and
// shares each with the block of the neighbouring node range.  Blocks are dealt round-robin to the 8 XCDs (one L2 each): with the
// plain (x, y) order the two halves of a line are fetched (written) by two different L2s -- measured 3.72 GB read for 2.12 GB of
// input.  Remapped, the blocks of one XCD cover a CONTIGUOUS range of (group, node block): the neighbour that shares a line runs
// on the same XCD a few blocks later and finds it in that L2.
__device__ __forceinline__ void xcd_block(int &bx, int &by) {
    const int gx = (int)gridDim.x, total = gx * (int)gridDim.y, lin = (int)blockIdx.y * gx + (int)blockIdx.x;
    const int per = total / 8;
    int nl = lin;
    if (lin < per * 8) nl = (lin & 7) * per + (lin >> 3);         // (the last total % 8 blocks keep their place)
    bx = nl % gx; by = nl / gx;
}

__device__ __forceinline__ void transpose4x4(uint32_t (&d)[4]) {
    const uint32_t a = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), b = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);
    const uint32_t c = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), e = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    d[0] = __builtin_amdgcn_perm(c, a, 0x05040100u); d[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
    d[2] = __builtin_amdgcn_perm(e, b, 0x05040100u); d[3] = __builtin_amdgcn_perm(e, b, 0x07060302u);
}

}  // namespace lutldpc
