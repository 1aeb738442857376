// logit_bias and grammar (guided decoding) masks on the device, for gfx950.
//
// apply_logit_mods_kernel, in place on logits [T, V] fp32, row t:
//
//   masks [M, W] int32, W = ceil(V / 32): bit (v & 31) of word (v >> 5) set
//   means token v is allowed. mask_ids [T] int32 names the row's mask; an id
//   outside [0, M) (canonically -1) means "no mask" and is never used as an
//   index. Bits of the last word at positions >= V are ignored.
//
//   bias in CSR form: bias_cu [T + 1] int32, bias_ids [B] int32, bias_vals
//   [B] fp32; row t owns the entries [bias_cu[t], bias_cu[t + 1]), clamped
//   to [0, B). An id outside [0, V) is skipped and never used as an index.
//   Ids within a row are distinct (the host takes them from dict keys).
//
//   result = "bias, then mask":
//     v disallowed by the row's mask   x = -inf (0xFF800000), whatever it
//                                      held (NaN included) and whatever the
//                                      bias says
//     v allowed (or no mask), biased   x = x + bias_vals[e], one fp32 add
//     anything else                    not stored to
//
// Who writes which element. Grid (column tiles, T), the apply_penalties
// shape, so that one to eight rows still cover the CUs.
//   mask pass: the workgroup that owns the 2048-column tile, and there the
//     lane that owns the group of four columns, stores -inf to the
//     DISALLOWED columns of the group and to nothing else.
//   bias pass: entry e of the row belongs to exactly one thread of the row's
//     workgroups (entries are dealt round-robin over them); it tests the
//     mask bit itself and stores only to an ALLOWED column.
// The two sets of columns are disjoint and ids are distinct within a row,
// so no element has two writers and the result does not depend on the order
// in which workgroups run. No float atomics, no LDS, no workspace, no host
// sync: hipGraph-capturable. A row with neither a mask nor a bias entry
// returns before it touches logits.
//
// Access. The mask pass is write-mostly: it reads one mask word per 128 B of
// logits (eight lanes share the word, each owns 16 B) and never reads
// logits. A group whose four bits are all clear is one 16 B store when
// V % 4 == 0 and the base is 16 B aligned; a mixed group, and every group on
// the unaligned path (V = 4099), uses bounds-checked 4 B stores. A group
// whose bits are all set (every group of an all-ones word) costs nothing.

#include <hip/hip_runtime.h>

#include "common.h"

namespace fi {

namespace {

constexpr int kModThreads = 256;
constexpr int kModVec = 4;
constexpr int kModUnroll = 2;
constexpr int kModTile = kModThreads * kModVec * kModUnroll;

__global__ __launch_bounds__(kModThreads) void apply_logit_mods_kernel(
    float* __restrict__ logits, const int* __restrict__ mask_ids,
    const int* __restrict__ masks, const int* __restrict__ bias_cu,
    const int* __restrict__ bias_ids, const float* __restrict__ bias_vals,
    int V, int M, int W, int B, int vec_i) {
  const int t = blockIdx.y;
  // block-uniform: the row's mask (nullptr = none) and its bias entries
  const u32* __restrict__ mrow = nullptr;
  if (mask_ids != nullptr) {
    const int mid = mask_ids[t];
    if (static_cast<u32>(mid) < static_cast<u32>(M))
      mrow = reinterpret_cast<const u32*>(masks) + static_cast<size_t>(mid) * W;
  }
  int e_lo = 0, e_hi = 0;
  if (bias_cu != nullptr) {
    e_lo = max(bias_cu[t], 0);
    e_hi = min(bias_cu[t + 1], B);
  }
  if (mrow == nullptr && e_lo >= e_hi) return;

  float* __restrict__ row = logits + static_cast<size_t>(t) * V;
  const float ninf = __int_as_float(static_cast<int>(0xFF800000u));

  if (mrow != nullptr) {
    const int base = blockIdx.x * kModTile + threadIdx.x * kModVec;
    u32 bits[kModUnroll];
#pragma unroll
    for (int u = 0; u < kModUnroll; ++u) {
      // i is a multiple of 4: its four columns share the word i >> 5, and
      // i < V gives i >> 5 < W
      const int i = base + u * kModThreads * kModVec;
      bits[u] = 0xFu;
      if (i < V) bits[u] = (mrow[i >> 5] >> (i & 31)) & 0xFu;
    }
#pragma unroll
    for (int u = 0; u < kModUnroll; ++u) {
      const int i = base + u * kModThreads * kModVec;
      if (bits[u] == 0xFu) continue;  // all allowed, or outside the row
      if (vec_i != 0 && bits[u] == 0u) {
        // V % 4 == 0: the group is inside the row as a whole
        *reinterpret_cast<float4*>(row + i) =
            make_float4(ninf, ninf, ninf, ninf);
        continue;
      }
#pragma unroll
      for (int j = 0; j < kModVec; ++j) {
        if (i + j < V && ((bits[u] >> j) & 1u) == 0u) row[i + j] = ninf;
      }
    }
  }

  // bias: entry e_lo + k goes to thread k of the row (k over all of the
  // row's workgroups), then on in steps of the row's thread count
  const int stride = gridDim.x * kModThreads;
  for (int e = e_lo + blockIdx.x * kModThreads + threadIdx.x; e < e_hi;
       e += stride) {
    const int v = bias_ids[e];
    if (static_cast<u32>(v) >= static_cast<u32>(V)) continue;
    if (mrow != nullptr && ((mrow[v >> 5] >> (v & 31)) & 1u) == 0u) continue;
    row[v] = row[v] + bias_vals[e];
  }
}

}  // namespace

void launch_apply_logit_mods(float* logits, const int* mask_ids,
                             const int* masks, const int* bias_cu,
                             const int* bias_ids, const float* bias_vals,
                             int T, int V, int M, int W, int B,
                             hipStream_t stream) {
  const bool vec = V % kModVec == 0 &&
      reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  hipLaunchKernelGGL(apply_logit_mods_kernel,
                     dim3(ceil_div(V, kModTile), T), dim3(kModThreads), 0,
                     stream, logits, mask_ids, masks, bias_cu, bias_ids,
                     bias_vals, V, M, W, B, vec ? 1 : 0);
}

}  // namespace fi
