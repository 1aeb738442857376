// Draft acceptance of speculative decoding on the device, for gfx950.
//
// The proposers draft deterministically, so the draft distribution is
// one-hot and rejection sampling reduces to: sample every row of a span from
// the target distribution, accept draft j while the sample of row j equals
// it, and emit the first mismatching sample as the corrected token.
//
// spec_accept_kernel: sampled [R] int64 (one token per verification row),
// drafts [R] int64 (the draft checked at row r, -1 at a span's last row,
// which checks nothing), span_cu [S + 1] int32: span s owns the rows
// [cu[s], cu[s + 1]). With m = the longest prefix of the span on which
// sampled == drafts:
//
//   emitted[s, :m + 1] = sampled[cu[s] : cu[s] + m + 1], the rest of the
//   row -1;  n_emit[s] = m + 1.
//
// A span that is empty, longer than W rows, or not inside [0, R) gets
// n_emit = 0 and a row of -1; its bounds are never used as an index. The
// last row of a span can only be reached with every draft in front of it
// accepted, and it always ends the span whatever drafts[] holds there.
//
// One thread per span (a span has at most 17 rows and S is the number of
// drafted sequences of a step, at most a few dozen): the kernel exists to
// keep the comparison off the host, not for throughput. emitted and n_emit
// are two sections of one buffer, so one copy brings both to the host.

#include <hip/hip_runtime.h>

#include "common.h"

namespace fi {

namespace {

constexpr int kAcceptThreads = 64;

__global__ __launch_bounds__(kAcceptThreads) void spec_accept_kernel(
    int64_t* __restrict__ emitted, int* __restrict__ n_emit,
    const int64_t* __restrict__ sampled, const int64_t* __restrict__ drafts,
    const int* __restrict__ span_cu, int R, int S, int W) {
  const int s = blockIdx.x * kAcceptThreads + threadIdx.x;
  if (s >= S) return;
  const int lo = span_cu[s];
  const int hi = span_cu[s + 1];
  // lo >= 0 and hi <= R first: hi - lo cannot overflow after them
  const bool ok = lo >= 0 && hi <= R && hi > lo && hi - lo <= W;
  int64_t* __restrict__ out = emitted + static_cast<size_t>(s) * W;
  int n = 0;
  if (ok) {
    const int rows = hi - lo;
    bool open = true;
    for (int j = 0; j < rows; ++j) {
      if (!open) break;
      const int64_t tok = sampled[lo + j];
      out[j] = tok;
      n = j + 1;
      open = j + 1 < rows && tok == drafts[lo + j];
    }
  }
  for (int j = n; j < W; ++j) out[j] = -1;
  n_emit[s] = n;
}

}  // namespace

void launch_spec_accept(int64_t* emitted, int* n_emit, const int64_t* sampled,
                        const int64_t* drafts, const int* span_cu, int R,
                        int S, int W, hipStream_t stream) {
  hipLaunchKernelGGL(spec_accept_kernel, dim3(ceil_div(S, kAcceptThreads)),
                     dim3(kAcceptThreads), 0, stream, emitted, n_emit,
                     sampled, drafts, span_cu, R, S, W);
}

}  // namespace fi
