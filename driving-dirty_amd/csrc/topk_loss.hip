// The bootstrapped road-map loss (include/dd_topk_loss.h; csrc/libdd_topk_loss.so, a library of its own): BCE-with-logits averaged
// over each sample's K hardest pixels, the K-th largest margin found by an exact radix select on the device.
//   dd_topk_bce / dd_topk_bce_u8_ptrs   the loss on a stacked byte target / on a host table of per-sample masks
// The launches of one call, all on the caller's stream:
//   topk_init_kernel                     zeroes the samples' histograms, writes the state blocks {prefix 0, rank K, n P}
//   topk_hist_kernel<D> + topk_select_kernel, for the digits D = 0, 1, 2 (11, 11, 10 bits of the key, from the top)
//   topk_final_kernel<Target, GRAD>      the loss pass: probabilities, the selected and the all-elements sums, the gradient
//   topk_finish_kernel                   stats and loss_out in a fixed order
// With keep == per_sample only the first (state blocks alone) and the last two.  The plan of the streaming passes is rm_loss.hip's
// (what they share is dd_loss_stats.h): a workgroup takes one piece of kChunk elements of ONE sample, in runs of kRun 16-byte vectors
// per lane whose loads are all issued before the first use; vectors past the end of the sample are clamped to its last vector for
// the load and skipped afterwards, so no load is behind a branch.
// COUNTS are integers: LDS atomics per workgroup, then one global integer atomic per non-zero bin.  Margins cluster -- on the leading
// digit (sign, exponent, two mantissa bits) most of a wave's lanes hit a handful of bins, and per-lane LDS atomics on one address
// serialise -- so a wave first PEELS: up to kPeel times the first remaining lane's digit is broadcast, the lanes that hold the same
// digit are counted by ballot and added ONCE; what is left after that adds per lane.  Every element in one bin costs one round; a
// spread digit costs kPeel cheap rounds and then finds few conflicts.  No floating-point atomics: every fp sum has a fixed order.
#include <limits.h>
#include <math.h>

#include "dd_loss_stats.h"

#include "../../include/dd_topk_loss.h"

#pragma clang fp contract(off)      // sp = max(u, 0) + l1p and sig - t are single rounded operations, never fused with their neighbours

namespace {

constexpr int kChunk = DD_TOPK_CHUNK, kTableMax = DD_TOPK_TABLE_MAX, kThreads = 256, kUnroll = kChunk / (4 * kThreads);
constexpr int kRun = 4;                    // vectors whose loads are in flight together
constexpr int kDigits = 3;
constexpr int kBits[kDigits] = {11, 11, 10}, kShift[kDigits] = {21, 10, 0}, kFirstBin[kDigits] = {0, 2048, 4096};
constexpr int kMaxBins = 2048, kBinsTotal = DD_TOPK_BINS;
constexpr int kPeel = 4;                   // rounds of wave aggregation before the per-lane atomics
constexpr int kFinishThreads = 1024;       // the finishing launch: one workgroup of sixteen waves, a wave per sample in turn
static_assert(kUnroll % kRun == 0 && kUnroll * 4 * kThreads == kChunk && kChunk % 1024 == 0, "a piece is a whole number of runs");
static_assert(kBits[0] + kBits[1] + kBits[2] == 32 && kFirstBin[2] + (1 << kBits[2]) == kBinsTotal, "the digits cover the key");
static_assert(DD_TOPK_PIECE_BYTES == 24 && DD_TOPK_STATE_BYTES == 16, "two fp64 sums and one 8-byte key per piece; four words per sample");

// per sample in the workspace: what the selection has found so far
struct State {
  unsigned prefix;      // the digits found so far, in place; after the last digit key(tau_b)
  unsigned rank;        // the remaining rank among the elements whose higher digits equal the prefix, 1-based
  unsigned n;           // n_b, once the last digit is found (per_sample before that: what keep == per_sample uses)
  unsigned pad;
};

// ---- the two forms of the target: where sample b's bytes lie
struct TargetU8 {
  const unsigned char* t;
  __device__ __forceinline__ const unsigned char* sample(int b, long per) const { return t + (long)b * per; }
};
struct TargetPtrs {      // by value in the kernel arguments
  const unsigned char* p[kTableMax];
  __device__ __forceinline__ const unsigned char* sample(int b, long) const { return p[b]; }
};

// key of the margin of logit bits `z` under label byte `t`, and the margin's own bits: a sign flip, -0 taken as +0
__device__ __forceinline__ unsigned margin_bits(unsigned z, unsigned t) {
  const unsigned u = z ^ (t ? 0x80000000u : 0u);
  return u == 0x80000000u ? 0u : u;
}
__device__ __forceinline__ unsigned key_of(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned bits_of_key(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// the fp32 value of `bits` as fp64 without a float instruction on a denormal: exact in every float mode
__device__ __forceinline__ double f64_of_bits(unsigned bits) {
  const unsigned mag = bits & 0x7fffffffu;
  const double v = (mag >> 23) == 0 ? (double)(int)mag * 0x1p-149 : (double)__builtin_bit_cast(float, mag);
  return (bits & 0x80000000u) ? -v : v;
}

// ---- init: the histograms zeroed, the state blocks written
__global__ __launch_bounds__(kThreads) void topk_init_kernel(unsigned* __restrict__ hist, long hist_words, State* __restrict__ state, int batch,
                                                             unsigned keep, unsigned per) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
  for (long j = i; j < hist_words; j += stride) hist[j] = 0u;
  for (long j = i; j < batch; j += stride) state[j] = State{0u, keep, per, 0u};
}

// One element's digit into the workgroup's LDS histogram: up to kPeel rounds of "the first remaining lane's digit, counted by ballot,
// added once", then per-lane atomics.  Called by all lanes of the wave; `active`: the lane has an element that takes part.
__device__ __forceinline__ void hist_add(unsigned* lds, unsigned digit, bool active, int lane) {
  unsigned long long todo = __ballot(active);
#pragma unroll 1
  for (int r = 0; r < kPeel && todo; ++r) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
    const bool same = active && digit == d0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&lds[d0], (unsigned)__popcll(m));
    active = active && !same;
    todo &= ~m;
  }
  if (active) atomicAdd(&lds[digit], 1u);
}

// grid = batch * pps workgroups; workgroup g takes piece g % pps of sample g / pps and adds the counts of digit D among the
// elements whose higher digits equal the sample's prefix to hist[kFirstBin[D] * batch + b * bins ..].
template <int D, typename Target>
__global__ __launch_bounds__(kThreads) void topk_hist_kernel(const float* __restrict__ logits, const Target target, long per, int pps, int batch,
                                                             const State* __restrict__ state, unsigned* __restrict__ hist) {
  constexpr int bins = 1 << kBits[D], shift = kShift[D], above = kShift[D > 0 ? D - 1 : 0], first = kFirstBin[D];
  __shared__ unsigned lds[bins];
  const int b = blockIdx.x / pps, piece = blockIdx.x - b * pps, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < bins; i += kThreads) lds[i] = 0u;
  const unsigned prefix = D == 0 ? 0u : state[b].prefix;
  const unsigned* __restrict__ zs = (const unsigned*)(logits + (long)b * per);
  const unsigned char* __restrict__ ts = target.sample(b, per);
  const long i0 = (long)piece * kChunk + 4 * threadIdx.x;
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < kUnroll; r += kRun) {
    u32x4 zv[kRun];
    unsigned tv[kRun];
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
      const long i = min(i0 + (long)(r + u) * 4 * kThreads, per - 4);      // past the end: the last vector again, loaded and not counted
      zv[u] = *(const u32x4*)(zs + i);
      tv[u] = *(const unsigned*)(ts + i);
    }
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
      const bool valid = i0 + (long)(r + u) * 4 * kThreads < per;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned key = key_of(margin_bits(zv[u][k], (tv[u] >> (8 * k)) & 0xffu));
        bool active = valid;
        if constexpr (D > 0) active = active && (key >> above) == (prefix >> above);
        hist_add(lds, (key >> shift) & (unsigned)(bins - 1), active, lane);
      }
    }
  }
  __syncthreads();
  unsigned* __restrict__ out = hist + (long)first * batch + (long)b * bins;
  for (int i = threadIdx.x; i < bins; i += kThreads) {
    const unsigned c = lds[i];
    if (c) atomicAdd(out + i, c);
  }
}

// grid = batch workgroups.  Thread i owns the bins_per_thread bins below bins - i * bins_per_thread, so ascending threads walk the bins
// from the top; an exclusive scan of the threads' counts finds the one thread whose bins hold the remaining rank, and that thread
// walks them.  It writes the digit into the prefix and the rank that remains inside the bin; after the last digit also n_b.
__global__ __launch_bounds__(kThreads) void topk_select_kernel(const unsigned* __restrict__ hist, int bins, int shift, int last, unsigned keep,
                                                               State* __restrict__ state) {
  __shared__ unsigned wave_total[kThreads / 64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per_thread = bins / kThreads;      // 8 or 4
  const unsigned* __restrict__ h = hist + (long)b * bins;
  const int top = bins - 1 - (int)threadIdx.x * per_thread;      // this thread's highest bin
  unsigned c[kMaxBins / kThreads], sum = 0;
#pragma unroll
  for (int k = 0; k < kMaxBins / kThreads; ++k) {
    c[k] = k < per_thread ? h[top - k] : 0u;
    sum += c[k];
  }
  unsigned incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  unsigned above = incl - sum;      // the count in the bins above this thread's
  for (int w = 0; w < wave; ++w) above += wave_total[w];
  const unsigned rank = state[b].rank;
  if (above < rank && rank <= above + sum) {      // one thread: the counts add up to at least the rank
#pragma unroll
    for (int k = 0; k < kMaxBins / kThreads; ++k) {
      if (k < per_thread && above < rank && rank <= above + c[k]) {
        const unsigned r = rank - above;
        state[b].prefix |= (unsigned)(top - k) << shift;
        state[b].rank = r;
        if (last) state[b].n = (keep - r) + c[k];
      }
      above += c[k];
    }
  }
}

// THE per-vector function of the final pass.  g = grad_scale / (B n_b); tkey = key(tau_b).
template <bool GRAD>
__device__ __forceinline__ void final_quad(const u32x4 zb, unsigned tw, unsigned tkey, float g, float& s_sel, float& s_all, unsigned& kmin, f32x4& p,
                                           f32x4& dz) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned zk = zb[k];      // a scalar copy: a bit cast of the vector element itself reads element 0
    const unsigned t = (tw >> (8 * k)) & 0xffu, ub = margin_bits(zk, t), key = key_of(ub);
    const float z = __builtin_bit_cast(float, zk), u = __builtin_bit_cast(float, ub);
    float sig, l1p;
    dd_sigmoid_softplus(z, sig, l1p);
    const float sp = fmaxf(u, 0.f) + l1p;
    const bool sel = key >= tkey;
    s_all += sp;
    s_sel += sel ? sp : 0.f;
    kmin = min(kmin, key);
    p[k] = sig;
    if constexpr (GRAD) dz[k] = sel ? g * (sig - (t ? 1.f : 0.f)) : 0.f;
  }
}

// grid = batch * pps workgroups, the pieces of the histogram passes.  Writes the piece's two fp64 sums and its smallest key.
template <typename Target, bool GRAD>
__global__ __launch_bounds__(kThreads) void topk_final_kernel(const float* __restrict__ logits, const Target target, long per, int pps, int batch,
                                                              float grad_scale, const State* __restrict__ state, float* __restrict__ probs,
                                                              float* __restrict__ dlogits, double* __restrict__ sums,
                                                              unsigned long long* __restrict__ min_key) {
  __shared__ unsigned wave_min[kThreads / 64];
  const int b = blockIdx.x / pps, piece = blockIdx.x - b * pps;
  const unsigned tkey = state[b].prefix;
  const float g = GRAD ? (float)((double)grad_scale / ((double)batch * (double)state[b].n)) : 0.f;
  const unsigned* __restrict__ zs = (const unsigned*)(logits + (long)b * per);
  const unsigned char* __restrict__ ts = target.sample(b, per);
  float* __restrict__ ps = probs ? probs + (long)b * per : nullptr;
  float* __restrict__ ds = GRAD ? dlogits + (long)b * per : nullptr;
  const long i0 = (long)piece * kChunk + 4 * threadIdx.x;
  float s_sel = 0.f, s_all = 0.f;
  unsigned kmin = 0xffffffffu;
#pragma unroll 1                  // one run's registers, not the piece's
  for (int r = 0; r < kUnroll; r += kRun) {
    u32x4 zv[kRun];
    unsigned tv[kRun];
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
      const long i = min(i0 + (long)(r + u) * 4 * kThreads, per - 4);      // past the end: the last vector again, loaded and not used
      zv[u] = *(const u32x4*)(zs + i);
      tv[u] = *(const unsigned*)(ts + i);
    }
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
      const long i = i0 + (long)(r + u) * 4 * kThreads;
      if (i < per) {              // i and per are multiples of 4: i + 4 <= per
        f32x4 p, dz;
        final_quad<GRAD>(zv[u], tv[u], tkey, g, s_sel, s_all, kmin, p, dz);
        if (ps) *(f32x4*)(ps + i) = p;
        if constexpr (GRAD) *(f32x4*)(ds + i) = dz;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (unsigned)__shfl_down(kmin, o));
  if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = kmin;
  const double acc[2] = {(double)s_sel, (double)s_all};
  dd_block_sum<2, kThreads>(acc, sums + 2L * blockIdx.x);      // its barrier also publishes wave_min
  if (threadIdx.x == 0) min_key[blockIdx.x] = min(min(wave_min[0], wave_min[1]), min(wave_min[2], wave_min[3]));
}

// One workgroup of sixteen waves; wave v takes the samples v, v + 16, ...: lane l adds the partials of pieces l, l + 64, ... of the
// sample, the lanes are added by shuffle, lane 0 writes the sample's statistics and keeps the wave's share of the two losses; thread 0
// adds the sixteen shares in order.  `all`: keep == per_sample, tau_b is the sample's smallest margin.
__global__ __launch_bounds__(kFinishThreads) void topk_finish_kernel(const double* __restrict__ sums, const unsigned long long* __restrict__ min_key,
                                                                     const State* __restrict__ state, int batch, int pps, double per, int all,
                                                                     double* __restrict__ stats, float* __restrict__ loss_out) {
  constexpr int kWaves = kFinishThreads / 64;
  __shared__ double red[2][kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double sel = 0.0, tot = 0.0;
  for (int b = wave; b < batch; b += kWaves) {
    double v[2] = {0.0, 0.0};
    dd_sample_sum(sums, b, pps, lane, v);
    unsigned kmin = 0xffffffffu;
    for (int j = lane; j < pps; j += 64) kmin = min(kmin, (unsigned)min_key[(long)b * pps + j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (unsigned)__shfl_down(kmin, o));
    if (lane == 0) {
      const double n = (double)state[b].n;
      stats[4L * b] = n;
      stats[4L * b + 1] = v[0];
      stats[4L * b + 2] = f64_of_bits(bits_of_key(all ? kmin : state[b].prefix));
      stats[4L * b + 3] = v[1];
      sel += v[0] / n;
      tot += v[1];
    }
  }
  if (lane == 0) {
    red[0][wave] = sel;
    red[1][wave] = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0, a = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      s += red[0][w];
      a += red[1][w];
    }
    loss_out[0] = (float)(s / (double)batch);
    loss_out[1] = (float)(a / ((double)batch * per));
  }
}

// ---- the host side: every refusal before any device call
bool overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

int pieces_per_sample(int64_t per) { return (int)((per + kChunk - 1) / kChunk); }      // < 2^18: per < 2^31

int check(const char* who, const float* logits, int32_t batch, int64_t per, int64_t keep, float grad_scale, const float* probs,
          const float* dlogits, const float* loss_out, const double* stats, const void* workspace, int64_t workspace_bytes) {
  DD_REQUIRE(logits, DD_ERR_BAD_ARG, "%s: logits is NULL", who);
  DD_REQUIRE(loss_out, DD_ERR_BAD_ARG, "%s: loss_out is NULL", who);
  DD_REQUIRE(stats, DD_ERR_BAD_ARG, "%s: stats is NULL", who);
  DD_REQUIRE(workspace, DD_ERR_BAD_ARG, "%s: workspace is NULL", who);
  DD_REQUIRE(batch >= 1 && per > 0, DD_ERR_BAD_ARG, "%s: batch = %d and per_sample = %lld must be positive", who, batch, (long long)per);
  DD_REQUIRE(per % 4 == 0 && per < ((int64_t)1 << 31) && per <= ((int64_t)1 << 40) / batch, DD_ERR_UNSUPPORTED,
             "%s: per_sample = %lld must be a multiple of 4 below 2^31, batch * per_sample at most 2^40", who, (long long)per);
  DD_REQUIRE(keep >= 1 && keep <= per, DD_ERR_BAD_ARG, "%s: keep = %lld must be in 1 .. per_sample = %lld", who, (long long)keep, (long long)per);
  DD_REQUIRE((uintptr_t)logits % 16 == 0, DD_ERR_BAD_ARG, "%s: logits is not 16-byte aligned", who);
  DD_REQUIRE((uintptr_t)probs % 16 == 0, DD_ERR_BAD_ARG, "%s: probs is not 16-byte aligned", who);
  DD_REQUIRE((uintptr_t)dlogits % 16 == 0, DD_ERR_BAD_ARG, "%s: dlogits is not 16-byte aligned", who);
  DD_REQUIRE((uintptr_t)loss_out % 4 == 0, DD_ERR_BAD_ARG, "%s: loss_out is not 4-byte aligned", who);
  DD_REQUIRE((uintptr_t)stats % 8 == 0, DD_ERR_BAD_ARG, "%s: stats is not 8-byte aligned", who);
  DD_REQUIRE((uintptr_t)workspace % 8 == 0, DD_ERR_BAD_ARG, "%s: workspace is not 8-byte aligned", who);
  DD_REQUIRE(grad_scale - grad_scale == 0.f, DD_ERR_BAD_ARG, "%s: grad_scale = %g must be finite", who, (double)grad_scale);      // false for a NaN too
  const int64_t need = (int64_t)batch * ((int64_t)DD_TOPK_PIECE_BYTES * pieces_per_sample(per) + 4 * kBinsTotal + DD_TOPK_STATE_BYTES);
  DD_REQUIRE(workspace_bytes >= need, DD_ERR_BAD_ARG, "%s: workspace_bytes = %lld, %d x %lld elements need %lld", who,
             (long long)workspace_bytes, batch, (long long)per, (long long)need);
  DD_REQUIRE((int64_t)batch * pieces_per_sample(per) <= INT_MAX, DD_ERR_UNSUPPORTED, "%s: %d x %lld elements need too many workgroups", who,
             batch, (long long)per);
  const int64_t bytes = (int64_t)batch * per * 4;
  DD_REQUIRE(!probs || !overlap(probs, logits, bytes), DD_ERR_BAD_ARG, "%s: probs overlaps logits", who);
  DD_REQUIRE(!dlogits || !overlap(dlogits, logits, bytes), DD_ERR_BAD_ARG, "%s: dlogits overlaps logits", who);
  DD_REQUIRE(!probs || !dlogits || !overlap(probs, dlogits, bytes), DD_ERR_BAD_ARG, "%s: probs overlaps dlogits", who);
  return 0;
}

int check_table(const char* who, const unsigned char* const* ptrs, int32_t batch, TargetPtrs& tab) {
  DD_REQUIRE(ptrs, DD_ERR_BAD_ARG, "%s: target_ptrs is NULL", who);
  DD_REQUIRE(batch <= kTableMax, DD_ERR_UNSUPPORTED, "%s: batch = %d, a pointer table holds at most %d samples", who, batch, kTableMax);
  for (int i = 0; i < kTableMax; ++i) tab.p[i] = i < batch ? ptrs[i] : nullptr;
  for (int i = 0; i < batch; ++i) {
    DD_REQUIRE(tab.p[i], DD_ERR_BAD_ARG, "%s: target_ptrs[%d] is NULL", who, i);
    DD_REQUIRE((uintptr_t)tab.p[i] % 4 == 0, DD_ERR_BAD_ARG, "%s: target_ptrs[%d] is not 4-byte aligned", who, i);
  }
  return 0;
}

template <int D, typename Target>
int launch_digit(const char* who, const float* logits, const Target& target, int32_t batch, int64_t per, int pps, int64_t keep, State* state,
                 unsigned* hist, hipStream_t st) {
  hipLaunchKernelGGL((topk_hist_kernel<D, Target>), dim3((unsigned)((long)batch * pps)), dim3(kThreads), 0, st, logits, target, (long)per, pps,
                     (int)batch, (const State*)state, hist);
  DD_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(topk_select_kernel, dim3((unsigned)batch), dim3(kThreads), 0, st, (const unsigned*)(hist + (long)kFirstBin[D] * batch),
                     1 << kBits[D], kShift[D], (int)(D == kDigits - 1), (unsigned)keep, state);
  DD_LAUNCH_CHECK(who);
  return 0;
}

template <typename Target>
int launch(const char* who, const float* logits, const Target& target, int32_t batch, int64_t per, int64_t keep, float grad_scale, float* probs,
           float* dlogits, float* loss_out, double* stats, void* workspace, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const int pps = pieces_per_sample(per);
  const long pieces = (long)batch * pps;
  // the workspace: the pieces' sums, their smallest keys, the histograms, the state blocks
  double* sums = (double*)workspace;
  unsigned long long* min_key = (unsigned long long*)(sums + 2 * pieces);
  unsigned* hist = (unsigned*)(min_key + pieces);
  State* state = (State*)(hist + (long)kBinsTotal * batch);
  const bool all = keep == per;      // every pixel is kept: no selection
  const long hist_words = all ? 0 : (long)kBinsTotal * batch;
  hipLaunchKernelGGL(topk_init_kernel, dim3((unsigned)dd_grid_for(max(hist_words, (long)batch))), dim3(kThreads), 0, st, hist, hist_words, state,
                     (int)batch, (unsigned)keep, (unsigned)per);
  DD_LAUNCH_CHECK(who);
  if (!all) {
    if (int rc = launch_digit<0>(who, logits, target, batch, per, pps, keep, state, hist, st)) return rc;
    if (int rc = launch_digit<1>(who, logits, target, batch, per, pps, keep, state, hist, st)) return rc;
    if (int rc = launch_digit<2>(who, logits, target, batch, per, pps, keep, state, hist, st)) return rc;
  }
  const dim3 grid((unsigned)pieces), block(kThreads);
  if (dlogits)
    hipLaunchKernelGGL((topk_final_kernel<Target, true>), grid, block, 0, st, logits, target, (long)per, pps, (int)batch, grad_scale,
                       (const State*)state, probs, dlogits, sums, min_key);
  else
    hipLaunchKernelGGL((topk_final_kernel<Target, false>), grid, block, 0, st, logits, target, (long)per, pps, (int)batch, grad_scale,
                       (const State*)state, probs, dlogits, sums, min_key);
  DD_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(topk_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, (const double*)sums, (const unsigned long long*)min_key,
                     (const State*)state, (int)batch, pps, (double)per, (int)all, stats, loss_out);
  DD_LAUNCH_CHECK(who);
  return 0;
}

}  // namespace

extern "C" {

int dd_topk_bce(const float* logits, const unsigned char* target, int32_t batch, int64_t per_sample, int64_t keep, float grad_scale,
                float* probs, float* dlogits, float* loss_out, double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "topk_bce";
  if (int rc = check(who, logits, batch, per_sample, keep, grad_scale, probs, dlogits, loss_out, stats, workspace, workspace_bytes)) return rc;
  DD_REQUIRE(target, DD_ERR_BAD_ARG, "%s: target is NULL", who);
  DD_REQUIRE((uintptr_t)target % 4 == 0, DD_ERR_BAD_ARG, "%s: target is not 4-byte aligned", who);
  return launch(who, logits, TargetU8{target}, batch, per_sample, keep, grad_scale, probs, dlogits, loss_out, stats, workspace, stream);
}

int dd_topk_bce_u8_ptrs(const float* logits, const unsigned char* const* target_ptrs, int32_t batch, int64_t per_sample, int64_t keep,
                        float grad_scale, float* probs, float* dlogits, float* loss_out, double* stats, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  const char* who = "topk_bce_u8_ptrs";
  TargetPtrs tab;
  if (int rc = check(who, logits, batch, per_sample, keep, grad_scale, probs, dlogits, loss_out, stats, workspace, workspace_bytes)) return rc;
  if (int rc = check_table(who, target_ptrs, batch, tab)) return rc;
  return launch(who, logits, tab, batch, per_sample, keep, grad_scale, probs, dlogits, loss_out, stats, workspace, stream);
}

}  // extern "C"
