// Repetition / presence / frequency penalties from a device-resident token
// histogram, for gfx950.
//
//   counts [S, V] int32: row s holds, per token, how often it occurs in the
//   (prompt + output) history of the sequence that owns slot s.
//
// apply_penalties_kernel, in place on logits [T, V] fp32, row t with
// slot = slot_ids[t] and (rp, inv_rp, presence, frequency) = params[t]:
//
//   slot outside [0, S)      row untouched, slot never used as an index
//   c = counts[slot][v] == 0 element untouched (no store)
//   c > 0                    x = x > 0 ? x * inv_rp : x * rp   (rp != 1)
//                            x = x - presence                  (presence != 0)
//                            x = x - frequency * float(c)      (frequency != 0)
//
// Each step is rounded to fp32 on its own (contraction off: frequency * c
// and the subtraction stay two roundings), which is the operation sequence
// of Sampler._apply_penalties on the GPU; inv_rp comes from the host: 1 / rp
// taken in double and rounded to fp32, which is what the torch build this
// was tested with multiplies by when it divides by a Python scalar on the
// GPU (found by experiment; tests/test_device_penalties_gpu.py is the
// judge after a torch upgrade). A skipped step and an
// executed one with the neutral value give the same bits, so the skips are
// only there to save work.
//
// Grid (column tiles, T): a row is spread over ceil(V / 2048) workgroups,
// so a batch of one to eight rows still covers the CUs. The histogram is
// read first; logits are only read where a group of four holds a nonzero
// count (a 1k-token history touches about 1k of 152k columns), and stores
// are per element. 16 B loads of both arrays when V % 4 == 0 and both
// bases are 16 B aligned, bounds-checked scalar accesses otherwise. No LDS,
// no atomics, no workspace, no host sync: hipGraph-capturable.
//
// apply_penalties_spec_kernel: the same for the rows of a speculative
// verification span, whose histories also hold the draft tokens in front of
// them (see the kernel).
//
// penalty_counts_add_kernel: counts[slot_ids[i]][token_ids[i]] += 1 with an
// integer atomicAdd (exact and order-independent for duplicates). A slot
// outside [0, S) or a token outside [0, V) is skipped and never used as an
// index.

#include <hip/hip_runtime.h>

#include "common.h"

namespace fi {

namespace {

constexpr int kPenThreads = 256;
constexpr int kPenVec = 4;
constexpr int kPenUnroll = 2;  // independent 16 B loads in flight per thread
constexpr int kPenTile = kPenThreads * kPenVec * kPenUnroll;
constexpr int kSpecMaxDraft = 16;  // ops.SPEC_MAX_DRAFT: extra ids per row

FI_DEV float penalise(float x, int c, float rp, float inv_rp, float presence,
                      float frequency) {
#pragma clang fp contract(off)
  if (rp != 1.0f) x = x > 0.0f ? x * inv_rp : x * rp;
  if (presence != 0.0f) x = x - presence;
  if (frequency != 0.0f) {
    const float f = frequency * static_cast<float>(c);
    x = x - f;
  }
  return x;
}

__global__ __launch_bounds__(kPenThreads) void apply_penalties_kernel(
    float* __restrict__ logits, const int* __restrict__ counts,
    const int* __restrict__ slot_ids, const float* __restrict__ params,
    int V, int S, int vec_i) {
  const int t = blockIdx.y;
  const int slot = slot_ids[t];
  if (static_cast<u32>(slot) >= static_cast<u32>(S)) return;
  const float rp = params[4 * t];
  const float inv_rp = params[4 * t + 1];
  const float presence = params[4 * t + 2];
  const float frequency = params[4 * t + 3];
  if (rp == 1.0f && presence == 0.0f && frequency == 0.0f) return;

  float* __restrict__ row = logits + static_cast<size_t>(t) * V;
  const int* __restrict__ crow = counts + static_cast<size_t>(slot) * V;
  const int base = blockIdx.x * kPenTile + threadIdx.x * kPenVec;

  if (vec_i != 0) {
    // V % 4 == 0: a group of four is inside the row or outside, never across
    int4 c[kPenUnroll];
#pragma unroll
    for (int u = 0; u < kPenUnroll; ++u) {
      const int i = base + u * kPenThreads * kPenVec;
      c[u] = make_int4(0, 0, 0, 0);
      if (i < V) c[u] = *reinterpret_cast<const int4*>(crow + i);
    }
#pragma unroll
    for (int u = 0; u < kPenUnroll; ++u) {
      const int i = base + u * kPenThreads * kPenVec;
      if ((c[u].x | c[u].y | c[u].z | c[u].w) == 0) continue;
      const float4 x = *reinterpret_cast<const float4*>(row + i);
      if (c[u].x != 0)
        row[i] = penalise(x.x, c[u].x, rp, inv_rp, presence, frequency);
      if (c[u].y != 0)
        row[i + 1] = penalise(x.y, c[u].y, rp, inv_rp, presence, frequency);
      if (c[u].z != 0)
        row[i + 2] = penalise(x.z, c[u].z, rp, inv_rp, presence, frequency);
      if (c[u].w != 0)
        row[i + 3] = penalise(x.w, c[u].w, rp, inv_rp, presence, frequency);
    }
  } else {
#pragma unroll
    for (int u = 0; u < kPenUnroll; ++u) {
      const int i = base + u * kPenThreads * kPenVec;
#pragma unroll
      for (int j = 0; j < kPenVec; ++j) {
        if (i + j >= V) continue;
        const int cj = crow[i + j];
        if (cj != 0)
          row[i + j] =
              penalise(row[i + j], cj, rp, inv_rp, presence, frequency);
      }
    }
  }
}

// Number of a row's extra ids (LDS copy, -1 = none) that fall on each of
// the four columns base .. base + 3.
FI_DEV int4 extra_hits(const int* ids, int E, int base) {
  int4 h = make_int4(0, 0, 0, 0);
  for (int e = 0; e < E; ++e) {
    const int d = ids[e] - base;  // ids[e] >= -1 and base >= 0: no overflow
    h.x += d == 0;
    h.y += d == 1;
    h.z += d == 2;
    h.w += d == 3;
  }
  return h;
}

// apply_penalties_kernel for the rows of a speculative verification span:
// row r of the span also counts the draft tokens in front of it, extra[r]
// ([E] int64, -1 = padding), so its effective count is
//   c = counts[slot][v] + #{e : extra[r][e] == v}.
// Same grid, same two access paths, same penalise(). The E ids are read
// once per workgroup into LDS (ids outside [0, V) become -1 there and so
// never meet a column); every thread then compares them with its own eight
// columns, which needs no atomics and leaves `counts` as it is.
__global__ __launch_bounds__(kPenThreads) void apply_penalties_spec_kernel(
    float* __restrict__ logits, const int* __restrict__ counts,
    const int* __restrict__ slot_ids, const float* __restrict__ params,
    const int64_t* __restrict__ extra, int V, int S, int E, int vec_i) {
  __shared__ int ids[kSpecMaxDraft];
  const int t = blockIdx.y;
  // block-uniform exits, both in front of the barrier
  const int slot = slot_ids[t];
  if (static_cast<u32>(slot) >= static_cast<u32>(S)) return;
  const float rp = params[4 * t];
  const float inv_rp = params[4 * t + 1];
  const float presence = params[4 * t + 2];
  const float frequency = params[4 * t + 3];
  if (rp == 1.0f && presence == 0.0f && frequency == 0.0f) return;

  if (threadIdx.x < E) {
    const int64_t id = extra[static_cast<size_t>(t) * E + threadIdx.x];
    ids[threadIdx.x] =
        id >= 0 && id < static_cast<int64_t>(V) ? static_cast<int>(id) : -1;
  }
  __syncthreads();

  float* __restrict__ row = logits + static_cast<size_t>(t) * V;
  const int* __restrict__ crow = counts + static_cast<size_t>(slot) * V;
  const int base = blockIdx.x * kPenTile + threadIdx.x * kPenVec;

  if (vec_i != 0) {
    int4 c[kPenUnroll];
#pragma unroll
    for (int u = 0; u < kPenUnroll; ++u) {
      const int i = base + u * kPenThreads * kPenVec;
      c[u] = make_int4(0, 0, 0, 0);
      if (i < V) c[u] = *reinterpret_cast<const int4*>(crow + i);
    }
#pragma unroll
    for (int u = 0; u < kPenUnroll; ++u) {
      const int i = base + u * kPenThreads * kPenVec;
      // a valid id is < V, so a group at i >= V gets no hit and stays 0
      const int4 h = extra_hits(ids, E, i);
      const int cx = c[u].x + h.x, cy = c[u].y + h.y;
      const int cz = c[u].z + h.z, cw = c[u].w + h.w;
      if ((cx | cy | cz | cw) == 0) continue;
      const float4 x = *reinterpret_cast<const float4*>(row + i);
      if (cx != 0) row[i] = penalise(x.x, cx, rp, inv_rp, presence, frequency);
      if (cy != 0)
        row[i + 1] = penalise(x.y, cy, rp, inv_rp, presence, frequency);
      if (cz != 0)
        row[i + 2] = penalise(x.z, cz, rp, inv_rp, presence, frequency);
      if (cw != 0)
        row[i + 3] = penalise(x.w, cw, rp, inv_rp, presence, frequency);
    }
  } else {
#pragma unroll
    for (int u = 0; u < kPenUnroll; ++u) {
      const int i = base + u * kPenThreads * kPenVec;
      const int4 h = extra_hits(ids, E, i);
      const int hj[kPenVec] = {h.x, h.y, h.z, h.w};
#pragma unroll
      for (int j = 0; j < kPenVec; ++j) {
        if (i + j >= V) continue;
        const int cj = crow[i + j] + hj[j];
        if (cj != 0)
          row[i + j] =
              penalise(row[i + j], cj, rp, inv_rp, presence, frequency);
      }
    }
  }
}

__global__ __launch_bounds__(kPenThreads) void penalty_counts_add_kernel(
    int* __restrict__ counts, const int* __restrict__ slot_ids,
    const int64_t* __restrict__ token_ids, int N, int V, int S) {
  const int i = blockIdx.x * kPenThreads + threadIdx.x;
  if (i >= N) return;
  const int slot = slot_ids[i];
  const int64_t tok = token_ids[i];
  if (static_cast<u32>(slot) >= static_cast<u32>(S)) return;
  if (tok < 0 || tok >= static_cast<int64_t>(V)) return;
  atomicAdd(counts + static_cast<size_t>(slot) * V + static_cast<size_t>(tok),
            1);
}

}  // namespace

void launch_apply_penalties(float* logits, const int* counts,
                            const int* slot_ids, const float* params, int T,
                            int V, int S, hipStream_t stream) {
  const bool vec = V % kPenVec == 0 &&
      reinterpret_cast<uintptr_t>(logits) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(counts) % 16 == 0;
  hipLaunchKernelGGL(apply_penalties_kernel,
                     dim3(ceil_div(V, kPenTile), T), dim3(kPenThreads), 0,
                     stream, logits, counts, slot_ids, params, V, S,
                     vec ? 1 : 0);
}

void launch_apply_penalties_spec(float* logits, const int* counts,
                                 const int* slot_ids, const float* params,
                                 const int64_t* extra, int T, int V, int S,
                                 int E, hipStream_t stream) {
  const bool vec = V % kPenVec == 0 &&
      reinterpret_cast<uintptr_t>(logits) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(counts) % 16 == 0;
  hipLaunchKernelGGL(apply_penalties_spec_kernel,
                     dim3(ceil_div(V, kPenTile), T), dim3(kPenThreads), 0,
                     stream, logits, counts, slot_ids, params, extra, V, S, E,
                     vec ? 1 : 0);
}

void launch_penalty_counts_add(int* counts, const int* slot_ids,
                               const int64_t* token_ids, int N, int V, int S,
                               hipStream_t stream) {
  hipLaunchKernelGGL(penalty_counts_add_kernel, dim3(ceil_div(N, kPenThreads)),
                     dim3(kPenThreads), 0, stream, counts, slot_ids,
                     token_ids, N, V, S);
}

}  // namespace fi
