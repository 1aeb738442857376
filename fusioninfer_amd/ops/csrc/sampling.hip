// Fused token sampling for gfx950: temperature, top-k, top-p, min-p and a
// seeded draw in one launch, one workgroup (1024 threads) per logits row.
//
//   z_i = x_i / max(temperature, 1e-5),  m = max z,
//   w_i = (u64) floor(expf(z_i - m) * 2^32)          (fixed-point weight)
//
// Every mass is an INTEGER sum of w, so histogram adds (LDS u64 atomics),
// reductions and scans give the same bits in any order: the token depends
// only on the row, its parameters and its (seed, offset) pair — not on T,
// on the wave schedule or on the scan shape. A token more than ~22.18
// (32 ln 2) below the row max has w = 0 and cannot be drawn.
//
// Phases (a row runs only the ones it needs):
//  1. argmax pass (lowest index on ties). temperature == 0, or a row whose
//     max is not finite, ends here (an all -inf row returns 0).
//  2. top-k (0 < k < V): radix select of the k-th largest z over an
//     order-preserving u32 key of the float bits (sign flip for negatives),
//     11 + 11 + 10 bits, one row pass per level, count histogram in LDS.
//     Everything >= t_k is kept, boundary ties included.
//  3. top-p (p < 1): the same descent over u64 MASS histograms of the
//     top-k survivors: keep i iff the mass of survivors with z_j > z_i is
//     <= floor(p_fix * Z_k / 2^32), p_fix = floor(p * 2^32). Ties kept.
//     Both descents are one routine: "find the lowest key whose mass
//     strictly above is <= P" with weight 1, P = k - 1 for top-k.
//  4. min-p: keep i iff expf(z_i - m) >= min(min_p, 1); evaluated in the
//     final passes. Z = sum of kept w: the top-p descent already yields it
//     when min-p is off, otherwise one reduction pass.
//  5. draw: u = Philox4x32-10(key = seed, counter = (offset, 0, 0))[0],
//     r = (u * Z) >> 32; tiled block scan (4096 tokens per tile, running
//     carry) to the smallest kept index whose inclusive prefix exceeds r.
//     The tile holding r is known to every thread from the tile total, so
//     the exit is uniform.
//
// Static grid (T workgroups), no host sync, no global workspace, no global
// atomics: hipGraph-capturable. Rows are read with 16 B loads when V % 4
// == 0 and the base is 16 B aligned, with bounds-checked scalar loads
// otherwise; the next tile's load is issued before the current tile is
// processed. The first histogram level of a descent sees every element of
// the row: lanes of a wave that hit the same bin serialize in the LDS
// (typically a handful of bins per wave for broad logit distributions);
// later levels only add the elements under the selected prefix.
//
// NaN logits are outside the contract (never chosen by the argmax, weight
// 0); they cannot cause an out-of-bounds access.

#include <hip/hip_runtime.h>

#include "common.h"

namespace fi {

namespace {

using u64 = unsigned long long;

constexpr int kSampThreads = 1024;
constexpr int kSampWaves = kSampThreads / kWaveSize;
constexpr int kSampVec = 4;
constexpr int kSampTile = kSampThreads * kSampVec;
constexpr int kSampBins = 2048;  // 11-bit digit

struct SampShared {
  u64 hist[kSampBins];
  u64 wave_tot[2][kSampWaves];
  float red_val[kSampWaves];
  int red_idx[kSampWaves];
  u64 sel_acc;
  u64 sel_mass;
  u32 sel_bin;
};

// ascending order-preserving key of a float (no NaN handling needed)
FI_DEV u32 float_key(float z) {
  const u32 b = __float_as_uint(z);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// x / t with -0 folded into +0, so that float order and key order agree
FI_DEV float scaled(float x, float t) { return x / t + 0.0f; }

FI_DEV u64 weight_of(float e) {
  return e >= 1.0f ? (1ull << 32)
                   : static_cast<u64>(__float2uint_rz(e * 4294967296.0f));
}

FI_DEV u32 philox4x32_10_x(u32 c0, u32 c1, u32 k0, u32 k1) {
  u32 c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// f(index, x) for every element of the row, in no particular order.
template <typename F>
FI_DEV void for_each_elem(const float* __restrict__ row, int V, bool vec,
                          F&& f) {
  const int tid = threadIdx.x;
  if (vec) {
    const float4* __restrict__ row4 = reinterpret_cast<const float4*>(row);
    const int n4 = V >> 2;
    float4 cur = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < n4) cur = row4[tid];
    for (int i = tid; i < n4; i += kSampThreads) {
      const int nx = i + kSampThreads;
      float4 nxt = cur;
      if (nx < n4) nxt = row4[nx];
      f(4 * i, cur.x);
      f(4 * i + 1, cur.y);
      f(4 * i + 2, cur.z);
      f(4 * i + 3, cur.w);
      cur = nxt;
    }
  } else {
    for (int i = tid * kSampVec; i < V; i += kSampTile) {
#pragma unroll
      for (int j = 0; j < kSampVec; ++j)
        if (i + j < V) f(i + j, row[i + j]);
    }
  }
}

// The four tokens [i, i + 4) of a scan tile; past the row end reads as
// -inf (weight 0).
FI_DEV float4 load_tile4(const float* __restrict__ row, int i, int V,
                         bool vec) {
  const float ninf = -__builtin_inff();
  float4 v = make_float4(ninf, ninf, ninf, ninf);
  if (vec) {
    if (i < V) v = *reinterpret_cast<const float4*>(row + i);
  } else {
    if (i < V) v.x = row[i];
    if (i + 1 < V) v.y = row[i + 1];
    if (i + 2 < V) v.z = row[i + 2];
    if (i + 3 < V) v.w = row[i + 3];
  }
  return v;
}

FI_DEV u64 wave_incl_scan(u64 v, int lane) {
#pragma unroll
  for (int off = 1; off < kWaveSize; off <<= 1) {
    const u64 n = __shfl_up(v, off, kWaveSize);
    if (lane >= off) v += n;
  }
  return v;
}

// Inclusive block scan; *total gets the block sum. One barrier: successive
// calls without another barrier in between must alternate `buf`.
FI_DEV u64 block_incl_scan(u64 v, SampShared& sh, int buf, u64* total) {
  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
  const u64 incl = wave_incl_scan(v, lane);
  if (lane == kWaveSize - 1) sh.wave_tot[buf][wave] = incl;
  __syncthreads();
  u64 pre = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kSampWaves; ++i) {
    const u64 t = sh.wave_tot[buf][i];
    if (i < wave) pre += t;
    tot += t;
  }
  *total = tot;
  return incl + pre;
}

// Radix descent. Over the elements with key >= lower_key, weighted 1
// (MASS = false) or w_i (MASS = true), returns the lowest key t such that
// the weight of elements with key > t is <= P, and in *mass_ge the weight
// of elements with key >= t. MASS = false: P = bound. MASS = true:
// P = floor(bound * total / 2^32) with `bound` the 32-bit fixed-point p.
template <bool MASS>
FI_DEV u32 radix_descend(const float* __restrict__ row, int V, bool vec,
                         float t, float m, u32 lower_key, u64 bound,
                         SampShared& sh, u64* mass_ge) {
  const int tid = threadIdx.x;
  u32 prefix = 0;
  u64 acc = 0, P = bound, sel_mass = 0;
#pragma unroll 1
  for (int level = 0; level < 3; ++level) {
    const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
    const int hi_shift = level == 1 ? 21 : 10;  // bits fixed by prefix
    const u32 bin_mask = level == 2 ? 1023u : 2047u;
    sh.hist[tid] = 0;
    sh.hist[tid + kSampThreads] = 0;
    __syncthreads();
    for_each_elem(row, V, vec, [&](int, float x) {
      const float z = scaled(x, t);
      const u32 key = float_key(z);
      const bool in = key >= lower_key &&
          (level == 0 || (key >> hi_shift) == (prefix >> hi_shift));
      if (in) {
        const u64 w = MASS ? weight_of(expf(z - m)) : 1ull;
        if (w != 0) atomicAdd(&sh.hist[(key >> shift) & bin_mask], w);
      }
    });
    __syncthreads();
    // thread owns bins (b_hi, b_lo), descending over the block
    const int b_hi = kSampBins - 1 - 2 * tid, b_lo = b_hi - 1;
    const u64 h_hi = sh.hist[b_hi], h_lo = sh.hist[b_lo];
    u64 total;
    const u64 incl = block_incl_scan(h_hi + h_lo, sh, level & 1, &total);
    if (MASS && level == 0) P = __umul64hi(bound << 32, total);
    const u64 a_hi = acc + incl - (h_hi + h_lo);  // weight above b_hi
    const u64 a_lo = a_hi + h_hi;
    if (a_hi <= P && a_hi + h_hi > P) {
      sh.sel_bin = b_hi;
      sh.sel_acc = a_hi;
      sh.sel_mass = h_hi;
    } else if (a_lo <= P && a_lo + h_lo > P) {
      sh.sel_bin = b_lo;
      sh.sel_acc = a_lo;
      sh.sel_mass = h_lo;
    } else if (tid == kSampThreads - 1 && a_lo + h_lo <= P) {
      // everything fits under P: descend into bin 0
      sh.sel_bin = 0;
      sh.sel_acc = a_lo;
      sh.sel_mass = h_lo;
    }
    __syncthreads();
    prefix |= sh.sel_bin << shift;
    acc = sh.sel_acc;
    sel_mass = sh.sel_mass;
  }
  *mass_ge = acc + sel_mass;
  return prefix;
}

__global__ __launch_bounds__(kSampThreads) void sample_tokens_kernel(
    int64_t* __restrict__ out, const float* __restrict__ logits,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ min_p,
    const int64_t* __restrict__ rng, int V, int vec_i) {
  __shared__ SampShared sh;
  const int tid = threadIdx.x;
  const int lane = tid % kWaveSize;
  const int wave = tid / kWaveSize;
  const int r_i = blockIdx.x;
  const bool vec = vec_i != 0;
  const float* __restrict__ row = logits + static_cast<size_t>(r_i) * V;
  const float ninf = -__builtin_inff();

  // ---- 1. argmax, lowest index on ties
  float best = ninf;
  int bi = 0x7FFFFFFF;
  for_each_elem(row, V, vec, [&](int i, float x) {
    if (x > best || (x == best && i < bi)) {
      best = x;
      bi = i;
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, kWaveSize);
    const int oi = __shfl_xor(bi, off, kWaveSize);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    sh.red_val[wave] = best;
    sh.red_idx[wave] = bi;
  }
  __syncthreads();
  best = sh.red_val[0];
  bi = sh.red_idx[0];
#pragma unroll
  for (int i = 1; i < kSampWaves; ++i) {
    const float ov = sh.red_val[i];
    const int oi = sh.red_idx[i];
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  const float temp = temperature[r_i];
  const bool finite_max = best > ninf && best < __builtin_inff();
  if (temp == 0.0f || !finite_max) {
    if (tid == 0) out[r_i] = best > ninf ? bi : 0;
    return;
  }

  const float t = fmaxf(temp, 1e-5f);
  const float m = scaled(best, t);
  const int k = top_k[r_i];
  const float p = top_p[r_i];
  const float mp = fminf(min_p[r_i], 1.0f);
  const bool use_mp = mp > 0.0f;

  // ---- 2./3. thresholds
  u32 thr = 0;
  u64 Z = 0;
  bool have_z = false;
  if (k > 0 && k < V) {
    u64 unused;
    thr = radix_descend<false>(row, V, vec, t, m, 0u,
                               static_cast<u64>(k - 1), sh, &unused);
  }
  if (p < 1.0f) {
    const u64 p_fix =
        p > 0.0f ? static_cast<u64>(__float2uint_rz(p * 4294967296.0f)) : 0;
    u64 mass;
    const u32 thr_p =
        radix_descend<true>(row, V, vec, t, m, thr, p_fix, sh, &mass);
    thr = thr_p > thr ? thr_p : thr;
    if (!use_mp) {
      Z = mass;
      have_z = true;
    }
  }

  auto kept_weight = [&](float x) -> u64 {
    const float z = scaled(x, t);
    const float e = expf(z - m);
    const bool kept = float_key(z) >= thr && (!use_mp || e >= mp);
    return kept ? weight_of(e) : 0ull;
  };

  // ---- 4. Z = sum of kept weights
  if (!have_z) {
    u64 part = 0;
    for_each_elem(row, V, vec, [&](int, float x) { part += kept_weight(x); });
    // buffer 1: the last descent level (2) used buffer 0
    block_incl_scan(part, sh, 1, &Z);
  }

  // ---- 5. draw
  const u64 seed = static_cast<u64>(rng[2 * r_i]);
  const u64 offset = static_cast<u64>(rng[2 * r_i + 1]);
  const u32 u = philox4x32_10_x(
      static_cast<u32>(offset), static_cast<u32>(offset >> 32),
      static_cast<u32>(seed), static_cast<u32>(seed >> 32));
  const u64 r = __umul64hi(static_cast<u64>(u) << 32, Z);  // (u * Z) >> 32

  const int ntiles = (V + kSampTile - 1) / kSampTile;
  u64 carry = 0;
  float4 cur = load_tile4(row, tid * kSampVec, V, vec);
#pragma unroll 1
  for (int tile = 0; tile < ntiles; ++tile) {
    const int i0 = tile * kSampTile + tid * kSampVec;
    float4 nxt = cur;
    if (tile + 1 < ntiles) nxt = load_tile4(row, i0 + kSampTile, V, vec);
    const u64 w0 = kept_weight(cur.x), w1 = kept_weight(cur.y),
              w2 = kept_weight(cur.z), w3 = kept_weight(cur.w);
    const u64 s = w0 + w1 + w2 + w3;
    u64 total;
    const u64 incl = carry + block_incl_scan(s, sh, tile & 1, &total);
    if (carry + total > r) {
      // r falls in this tile, in exactly one thread's span
      const u64 excl = incl - s;
      if (excl <= r && r < incl) {
        int idx = i0 + 3;
        if (excl + w0 > r) {
          idx = i0;
        } else if (excl + w0 + w1 > r) {
          idx = i0 + 1;
        } else if (excl + w0 + w1 + w2 > r) {
          idx = i0 + 2;
        }
        out[r_i] = idx;
      }
      return;
    }
    carry += total;
    cur = nxt;
  }
  // unreachable for Z > 0 (r < Z); Z == 0 cannot happen with a finite max
  if (tid == 0) out[r_i] = bi;
}

// ---------------------------------------------------------------------------
// token_logprobs: log-softmax value of one token per row plus the k largest
// (id, logprob) pairs, k <= kLpMaxTop, one workgroup per row.
//
//   logZ = m + logf(S),  m = max x,  S = sum expf(x - m),  lp(i) = x_i - logZ
//
// S is a float sum in a FIXED order: per-thread partials over the thread's
// elements in index order (the same elements on the 16 B and on the scalar
// load path), a xor butterfly per wave, then the 16 wave sums added in wave
// order. A row's bits depend only on the row and V.
//
// Top entries, ordered by (logit descending, index ascending) on the input
// values with -0 folded into +0: the radix descent gives the k-th largest
// key t_k; one pass appends the (fewer than k) elements above t_k to a list
// in LDS in arrival order; a tiled index-order scan adds the lowest-index
// elements equal to t_k until the list holds k; k threads then rank the list
// by counting predecessors. The ids are an exact function of the inputs.
//
// No index is derived from data: list slots come from a bounded counter or a
// bounded rank, output columns from a count over at most k - 1 others, and
// the token id is range-checked before it forms an address. NaN / +inf logits
// are outside the contract but cannot cause an out-of-bounds access.

constexpr int kLpMaxTop = 32;

struct LpShared {
  int idx[kLpMaxTop];
  float val[kLpMaxTop];
  int n_above;
};

template <bool MAX>
FI_DEV float block_reduce_f32(float v, SampShared& sh) {
  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, kWaveSize);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  __syncthreads();  // readers of an earlier reduction are done
  if (lane == 0) sh.red_val[wave] = v;
  __syncthreads();
  float r = sh.red_val[0];
#pragma unroll
  for (int i = 1; i < kSampWaves; ++i)
    r = MAX ? fmaxf(r, sh.red_val[i]) : r + sh.red_val[i];
  return r;
}

__global__ __launch_bounds__(kSampThreads) void token_logprobs_kernel(
    float* __restrict__ chosen, int* __restrict__ top_ids,
    float* __restrict__ top_lp, const float* __restrict__ logits,
    const int64_t* __restrict__ token_ids, const int* __restrict__ num_top,
    int V, int W, int vec_i) {
  __shared__ SampShared sh;
  __shared__ LpShared ls;
  const int tid = threadIdx.x;
  const int r_i = blockIdx.x;
  const int want = num_top[r_i];
  if (want < 0) return;  // skipped row: nothing read, nothing written
  const bool vec = vec_i != 0;
  const float* __restrict__ row = logits + static_cast<size_t>(r_i) * V;
  const float ninf = -__builtin_inff();
  const int width = W < kLpMaxTop ? W : kLpMaxTop;
  int k = want < width ? want : width;
  k = k < V ? k : V;

  if (tid < kLpMaxTop) {
    ls.idx[tid] = -1;
    ls.val[tid] = ninf;
  }
  if (tid == 0) ls.n_above = 0;

  // ---- log-partition
  float part = ninf;
  for_each_elem(row, V, vec, [&](int, float x) { part = fmaxf(part, x); });
  const float m = block_reduce_f32<true>(part, sh);
  const bool none_finite = !(m > ninf);
  float logz = 0.0f;
  if (!none_finite) {
    part = 0.0f;
    for_each_elem(row, V, vec, [&](int, float x) { part += expf(x - m); });
    logz = m + logf(block_reduce_f32<false>(part, sh));
  }
  auto lp_of = [&](float x) { return none_finite ? ninf : x - logz; };

  if (tid == 0) {
    const int64_t tok = token_ids[r_i];
    float c = __builtin_nanf("");
    if (tok >= 0 && tok < static_cast<int64_t>(V)) c = lp_of(row[tok]);
    chosen[r_i] = c;
  }
  // columns past k: id -1, value -inf
  if (tid >= k && tid < W) {
    top_ids[static_cast<size_t>(r_i) * W + tid] = -1;
    top_lp[static_cast<size_t>(r_i) * W + tid] = ninf;
  }
  if (k == 0) return;

  // ---- k-th largest key (temperature 1: scaled() only folds -0)
  u64 unused;
  const u32 tk = radix_descend<false>(row, V, vec, 1.0f, 0.0f, 0u,
                                      static_cast<u64>(k - 1), sh, &unused);

  // ---- everything above t_k, in arrival order (fewer than k elements)
  for_each_elem(row, V, vec, [&](int i, float x) {
    const float z = scaled(x, 1.0f);
    if (float_key(z) > tk) {
      const int slot = atomicAdd(&ls.n_above, 1);
      if (slot < kLpMaxTop) {
        ls.idx[slot] = i;
        ls.val[slot] = z;
      }
    }
  });
  __syncthreads();
  const int n_above = ls.n_above < k - 1 ? ls.n_above : k - 1;
  const u64 need = static_cast<u64>(k - n_above);

  // ---- the lowest-index elements equal to t_k fill the rest
  const int ntiles = (V + kSampTile - 1) / kSampTile;
  u64 carry = 0;
  float4 cur = load_tile4(row, tid * kSampVec, V, vec);
#pragma unroll 1
  for (int tile = 0; tile < ntiles; ++tile) {
    const int i0 = tile * kSampTile + tid * kSampVec;
    float4 nxt = cur;
    if (tile + 1 < ntiles) nxt = load_tile4(row, i0 + kSampTile, V, vec);
    const float z[kSampVec] = {scaled(cur.x, 1.0f), scaled(cur.y, 1.0f),
                               scaled(cur.z, 1.0f), scaled(cur.w, 1.0f)};
    bool eq[kSampVec];
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < kSampVec; ++j) {
      // the pad past the row end reads as -inf and may equal t_k
      eq[j] = i0 + j < V && float_key(z[j]) == tk;
      s += eq[j] ? 1 : 0;
    }
    u64 total;
    const u64 incl = carry + block_incl_scan(s, sh, tile & 1, &total);
    u64 rank = incl - s;
#pragma unroll
    for (int j = 0; j < kSampVec; ++j) {
      if (eq[j]) {
        if (rank < need) {
          const int slot = n_above + static_cast<int>(rank);  // < k
          ls.idx[slot] = i0 + j;
          ls.val[slot] = z[j];
        }
        ++rank;
      }
    }
    carry += total;
    if (carry >= need) break;  // uniform: every thread has the tile total
    cur = nxt;
  }
  __syncthreads();

  // ---- rank the k entries: key descending, then index ascending
  if (tid < k) {
    const int my_i = ls.idx[tid];
    const float my_v = ls.val[tid];
    const u32 my_key = float_key(my_v);
    int pos = 0;
    for (int j = 0; j < k; ++j) {
      const u32 key = float_key(ls.val[j]);
      pos += (key > my_key || (key == my_key && ls.idx[j] < my_i)) ? 1 : 0;
    }
    top_ids[static_cast<size_t>(r_i) * W + pos] = my_i;
    top_lp[static_cast<size_t>(r_i) * W + pos] = lp_of(my_v);
  }
}

}  // namespace

void launch_sample_tokens(int64_t* out, const float* logits,
                          const float* temperature, const int* top_k,
                          const float* top_p, const float* min_p,
                          const int64_t* rng, int T, int V,
                          hipStream_t stream) {
  const bool vec =
      V % kSampVec == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  hipLaunchKernelGGL(sample_tokens_kernel, dim3(T), dim3(kSampThreads), 0,
                     stream, out, logits, temperature, top_k, top_p, min_p,
                     rng, V, vec ? 1 : 0);
}

void launch_token_logprobs(float* chosen, int* top_ids, float* top_lp,
                           const float* logits, const int64_t* token_ids,
                           const int* num_top, int T, int V, int W,
                           hipStream_t stream) {
  const bool vec =
      V % kSampVec == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(T), dim3(kSampThreads), 0,
                     stream, chosen, top_ids, top_lp, logits, token_ids,
                     num_top, V, W, vec ? 1 : 0);
}

}  // namespace fi
