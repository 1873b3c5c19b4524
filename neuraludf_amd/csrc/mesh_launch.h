// What the launchers of the mesh kernel files share: the block count of a one-dimensional grid, the refusal of a bad
// descriptor and the launch itself.  (Not in nudf_common.h: that header is part of the recorded source digests of the
// training kernels, which none of this concerns.)
#pragma once
#include "nudf_common.h"

static unsigned blocks(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// refuses a descriptor: nudf_last_error reads "<entry>: <why>: invalid argument"
static int refuse(const char* entry, const char* why) {
  char text[384];
  snprintf(text, sizeof(text), "%s: %s", entry, why);
  return nudf_refuse(text);                             // copies the text
}

// the tail of an entry point `entry` whose descriptor is `a` and whose stream is `stream`: `n` items, `per_block` of them
// to a block of `block` threads
#define MESH_LAUNCH(kernel, n, block, per_block, entry)                                                   \
  hipLaunchKernelGGL(kernel, dim3(blocks(n, per_block)), dim3(block), 0, (hipStream_t)stream, a);         \
  NUDF_CHECK_LAUNCH(entry);                                                                               \
  return 0
