// The sampled road-map head's uncertainty (include/dd_head_uncert.h; csrc/libdd_head_uncert.so, a library of its own):
//   dd_head_uncert   per pixel: the mean of the S draws' probabilities, the entropy of that mean, the mutual information (entropy minus
//                    the mean entropy of the draws) and the variance of the draws -> fp32 [scenes,n] each, any of them optional;
//                    per scene: the means of the last three over the pixels -> fp64 [scenes,3], optional
// One stream over the weight serves up to 64 rows = floor(64 / S) scenes x S draws, as head_mean.hip: the tiles and the contraction
// are linear.hip's (written out again below as fwd_tiles, as head_mean.hip writes them out), so the accumulators hold dd_linear_fwd's
// logit bits and `mean` dd_head_mean_prob's.
//
// THE EPILOGUE.  Every lane takes dd_sigmoid_softplus of its OWN accumulator elements -- all 256 lanes at work on the transcendentals,
// as in head_mean_kernel -- and gets from each logit the draw's probability p and the draw's entropy h = l1p + |z| q.  The S rows of a
// scene lie in different registers and lanes, so the block puts them together through a row-major fp32 tile [rows][128] in the LDS, in
// the weight's operand tile (32 KB of its 34 KB), twice over:
//   1. the h tile.  Lane (tid & 31) of thread row (tid >> 5) owns four consecutive columns of the scenes b = tid >> 5, + 8, ...: it
//      reads the S rows of a scene as 16-byte pieces (a half-wave reads one 512-byte row: every 16-lane group of ds_read_b128 on 64
//      distinct banks) and adds them in draw order.  `expected` stays in registers: at most 8 scenes per lane, a compile-time count.
//   2. the p tile, after a barrier.  The same lane adds the S probabilities in draw order (head_mean_kernel's loop: the same bits),
//      walks the rows a second time for the variance, and takes the entropy of the mean and the mutual information.
// No registers are traded between lanes for the sums over draws, no atomics, no scratch.
//
// THE SCORES.  The 32 lanes of a scene put their 4 columns x 3 statistics into a staging row set [3][128] in the activation operand
// tile; after a barrier lanes 0, 1, 2 add one statistic each over the block's valid columns in column order, widened to fp64, and store
// partials[block, scene, :].  head_uncert_finish -- one workgroup per scene -- brings the blocks' triples through the LDS and adds
// them in block order.  The staging and its two barriers are skipped when no scores are asked for; every other operation is the same
// code whatever is written, so the bits do not depend on which outputs were asked for.
#include "dd_common.h"

#include "../../include/dd_head_uncert.h"

#pragma clang fp contract(off)      // every add and multiply of the header's formulas is ONE rounded operation

namespace {

constexpr int KT = 64;          // k-chunk of the forward kernel
constexpr int WROW = KT + 4;    // LDS row stride in floats: 272 B keeps 16 rows x 16 B on 64 distinct banks
constexpr int BLOCK = DD_HEAD_UNCERT_BLOCK;
static_assert(BLOCK == 128, "a workgroup owns 128 columns: four waves of 32");

// linear.hip's forward contraction, written out again as in head_mean.hip (tests/test_gpu_head_uncert.py holds `mean` to
// dd_head_mean_prob's bits).  Y tile [MT*32 rows, 128 columns from n0] += X[M,K] W[N,K]^T over the k-tiles [t0, t1), 256 threads = 4
// waves, wave w owns the columns [n0 + 32w, +32).  `wl` (128 * WROW floats) and `xl` (MT * 32 * WROW floats) are the caller's LDS
// operand tiles, 16-byte aligned; the loop ends on a barrier, so they are free for the epilogue when this returns.  acc[mt][i] is the
// element of row mt * 32 + dd_acc_row(i, lane), column n0 + 32 * wave + (lane & 31); rows >= M and columns >= N hold exact zeros' products.
template <int MT>
__device__ __forceinline__ void fwd_tiles(const float* __restrict__ X, const float* __restrict__ Wt, int M, int N, int K, int n0, int t0, int t1,
                                          float* wl, float* xl, f32x16 (&acc)[MT], int tid, int wave) {
  const int lane = tid & 63;      // `tid` and `wave` are the caller's threadIdx.x and its readfirstlane(tid >> 6)
  const int h = lane >> 5, r = lane & 31;
  const int lrow = tid >> 4, lch = tid & 15;    // staging: 16 threads cover one 256-byte row segment

  f32x4 wreg[8], xreg[2 * MT];
  auto fetch = [&](int t) {
    const int kc = t * KT + lch * 4;
    const bool kok = kc < K;                    // K % 4 == 0 is required, so a chunk is all-in or all-out
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int n = n0 + p * 16 + lrow;
      const f32x4 v = __builtin_nontemporal_load((const f32x4*)(Wt + (long)min(n, N - 1) * K + min(kc, K - 4)));      // the weight streams through once
      wreg[p] = (kok && n < N) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int p = 0; p < 2 * MT; ++p) {
      const int m = p * 16 + lrow;
      const f32x4 v = *(const f32x4*)(X + (long)min(m, M - 1) * K + min(kc, K - 4));
      xreg[p] = (kok && m < M) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

  if (t0 < t1) fetch(t0);
  for (int t = t0; t < t1; ++t) {
#pragma unroll
    for (int p = 0; p < 8; ++p) *(f32x4*)(wl + (p * 16 + lrow) * WROW + lch * 4) = wreg[p];
#pragma unroll
    for (int p = 0; p < 2 * MT; ++p) *(f32x4*)(xl + (p * 16 + lrow) * WROW + lch * 4) = xreg[p];
    __syncthreads();
    if (t + 1 < t1) fetch(t + 1);               // next tile's HBM loads fly under this tile's MFMAs
#pragma unroll
    for (int s = 0; s < KT / 8; ++s) {
      const f32x4 b4 = *(const f32x4*)(wl + (wave * 32 + r) * WROW + 8 * s + 4 * h);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const f32x4 a4 = *(const f32x4*)(xl + (mt * 32 + r) * WROW + 8 * s + 4 * h);
        acc[mt] = DD_MFMA(a4.x, b4.x, acc[mt]);
        acc[mt] = DD_MFMA(a4.y, b4.y, acc[mt]);
        acc[mt] = DD_MFMA(a4.z, b4.z, acc[mt]);
        acc[mt] = DD_MFMA(a4.w, b4.w, acc[mt]);
      }
    }
    __syncthreads();
  }
}

// Over how many workgroups dd_linear_fwd splits a contraction of `ntiles` k-tiles when `blocks_other` workgroups cover the output
// (linear.hip's rule, as head_mean.hip restates it).  1 = one workgroup walks the whole contraction: dd_linear_fwd's own logit bits.
inline int pick_split(int blocks_other, int ntiles) {
  if (ntiles <= 8) return 1;
  int want = (2 * DD_NUM_CU + blocks_other - 1) / blocks_other;
  want = max(1, min(want, ntiles));
  return min(want, 512);
}

inline int pick_mt(int M) { return M <= 32 ? 1 : (M <= 64 ? 2 : 0); }
constexpr int MAX_ROWS = 64;      // rows of a launch: floor(64 / S) scenes of S draws
constexpr int STAGE = 8 * 3 * BLOCK;      // floats: one [3][128] row set per half-wave of the workgroup

// One term of the binary entropy: -(f ln f), 0 where the factor is 0; a NaN stays a NaN.
__device__ __forceinline__ float entropy_term(float f) { return f == 0.f ? 0.f : -(f * logf(f)); }

// grid ceil(N / 128); 4 waves.  X: the launch's nb * S rows; the maps: its nb rows (or null); partials: block stride `scenes` triples,
// offset to the launch's first scene (or null).
template <int MT>
__global__ __launch_bounds__(256) void head_uncert_kernel(const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                          float* __restrict__ mean, float* __restrict__ entropy, float* __restrict__ mi,
                                                          float* __restrict__ var, double* __restrict__ partials, int nb, int S, float inv, int N,
                                                          int K, int scenes) {
  constexpr int XL = MT * 32 * WROW > STAGE ? MT * 32 * WROW : STAGE;
  __shared__ __attribute__((aligned(16))) float wl[128 * WROW];
  __shared__ __attribute__((aligned(16))) float xl[XL];
  static_assert(MT * 32 * 128 <= 128 * WROW, "the h tile and the p tile lie, one after the other, in the weight's operand tile");
  constexpr int IT = MT * 4;      // scenes a gathering lane can own: at most MT * 32 scenes of a launch, 8 at a time
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31;
  const int n0 = blockIdx.x * BLOCK;

  f32x16 acc[MT];
  fwd_tiles<MT>(X, Wt, nb * S, N, K, n0, 0, (K + KT - 1) / KT, wl, xl, acc, tid, wave);

  const bool stats = entropy || mi || var || partials;      // uniform: anything beyond the mean
  const int n = n0 + wave * 32 + r;
  const float bv = (bias && n < N) ? bias[n] : 0.f;
  float* tile = wl;      // [MT*32][128]; rows past nb * S and columns past N hold the values of zero logits: finite, never read out
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float z = acc[mt][i] + bv;
      float sig, l1p;
      dd_sigmoid_softplus(z, sig, l1p);      // the dense head's one sigmoid
      acc[mt][i] = sig;
      if (stats) {
        const float az = fabsf(z);
        float q, l1q;
        dd_sigmoid_softplus(-az, q, l1q);      // the same exponential and reciprocal: q = sigmoid(-|z|), l1q = log1p(exp(-|z|))
        tile[(mt * 32 + dd_acc_row(i, lane)) * 128 + wave * 32 + r] = l1q + az * q;
      }
    }

  const int cg = tid & 31, c = 4 * cg;      // this lane's four columns of the tile
  const int hw = tid >> 5;                  // its half-wave: the scenes hw, hw + 8, ...
  f32x4 expected[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) expected[it] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (stats) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int b = it * 8 + hw;
      if (b < nb) {
        const float* row = tile + b * S * 128 + c;
        f32x4 sum = *(const f32x4*)row;
        for (int s = 1; s < S; ++s) sum += *(const f32x4*)(row + s * 128);      // draw order
        expected[it] = sum * inv;
      }
    }
    __syncthreads();      // the h tile is read: the p tile takes its place
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[(mt * 32 + dd_acc_row(i, lane)) * 128 + wave * 32 + r] = acc[mt][i];
  __syncthreads();

  float* stage = xl + hw * 3 * BLOCK;      // this half-wave's [3][128]
  const int cols = min(BLOCK, N - n0);
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    if (it * 8 >= nb) break;      // uniform
    const int b = it * 8 + hw;
    const bool on = b < nb;
    f32x4 m4 = {0.f, 0.f, 0.f, 0.f}, e4 = m4, i4 = m4, v4 = m4;
    if (on) {
      const float* row = tile + b * S * 128 + c;
      f32x4 sum = *(const f32x4*)row;
      for (int s = 1; s < S; ++s) sum += *(const f32x4*)(row + s * 128);      // draw order: head_mean_kernel's loop
      m4 = sum * inv;
      if (stats) {
        f32x4 d = *(const f32x4*)row - m4;
        v4 = d * d;
        for (int s = 1; s < S; ++s) {      // the second pass, draw order
          d = *(const f32x4*)(row + s * 128) - m4;
          v4 += d * d;
        }
        v4 = v4 * inv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          e4[j] = entropy_term(m4[j]) - (1.f - m4[j] == 0.f ? 0.f : (1.f - m4[j]) * logf(1.f - m4[j]));
          const float gap = e4[j] - expected[it][j];
          i4[j] = S == 1 ? 0.f * e4[j] : (gap < 0.f ? 0.f : gap);      // a NaN gap stays
        }
      }
      const long at = (long)b * N + n0 + c;
      if (N % 4 == 0) {      // then the four columns are all inside the row or all outside, and 16-byte aligned
        if (n0 + c < N) {
          if (mean) *(f32x4*)(mean + at) = m4;
          if (entropy) *(f32x4*)(entropy + at) = e4;
          if (mi) *(f32x4*)(mi + at) = i4;
          if (var) *(f32x4*)(var + at) = v4;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n0 + c + j < N) {
            if (mean) mean[at + j] = m4[j];
            if (entropy) entropy[at + j] = e4[j];
            if (mi) mi[at + j] = i4[j];
            if (var) var[at + j] = v4[j];
          }
      }
    }
    if (partials) {      // uniform
      if (on) {
        *(f32x4*)(stage + c) = e4;
        *(f32x4*)(stage + BLOCK + c) = i4;
        *(f32x4*)(stage + 2 * BLOCK + c) = v4;
      }
      __syncthreads();
      if (on && cg < 3) {
        const float* src = stage + cg * BLOCK;
        double total = 0.0;
        for (int j = 0; j < cols; j += 4) {      // column order
          const f32x4 v = *(const f32x4*)(src + j);
          total += (double)v.x;
          if (j + 1 < cols) total += (double)v.y;
          if (j + 2 < cols) total += (double)v.z;
          if (j + 3 < cols) total += (double)v.w;
        }
        partials[((long)blockIdx.x * scenes + b) * 3 + cg] = total;
      }
      __syncthreads();      // the staging rows are read: the next eight scenes may overwrite them
    }
  }
}

constexpr int FIN_CHUNK = 2048;      // blocks' triples a workgroup of the finishing launch holds in its 48 KB of LDS

// grid `scenes`; 256 threads.  scores[b, :] = (partials[0, b, :] + partials[1, b, :] + ...) / n, the blocks added in block order by lanes
// 0, 1, 2; the other lanes fetch: FIN_CHUNK triples at a time go through the LDS so that the adds do not each wait for a load.
__global__ __launch_bounds__(256) void head_uncert_finish(const double* __restrict__ partials, double* __restrict__ scores, int nblk, int scenes,
                                                          double n) {
  __shared__ double buf[FIN_CHUNK * 3];
  const int b = blockIdx.x, tid = threadIdx.x;
  double total = 0.0;
  for (int i0 = 0; i0 < nblk; i0 += FIN_CHUNK) {
    const int cnt = min(FIN_CHUNK, nblk - i0);
    for (int e = tid; e < cnt * 3; e += 256) buf[e] = partials[((long)(i0 + e / 3) * scenes + b) * 3 + e % 3];
    __syncthreads();
    if (tid < 3)
      for (int i = 0; i < cnt; ++i) total += buf[i * 3 + tid];      // block order
    __syncthreads();
  }
  if (tid < 3) scores[b * 3 + tid] = total / n;
}

bool overlaps(const void* p, long p_bytes, const void* q, long q_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}

struct Span {
  const void* p;
  long bytes;
  const char* name;
};

}  // namespace

extern "C" {

int dd_head_uncert(const float* x, const float* w, const float* bias, float* mean, float* entropy, float* mi, float* var, double* partials,
                   double* scores, int32_t scenes, int32_t samples, int32_t n, int32_t k, void* stream) {
  const char* who = "head_uncert";
  DD_REQUIRE(x && w, DD_ERR_BAD_ARG, "%s: NULL pointer", who);
  DD_REQUIRE(mean || entropy || mi || var || scores || partials, DD_ERR_BAD_ARG, "%s: no output requested (every map and scores are NULL)", who);
  DD_REQUIRE((partials != nullptr) == (scores != nullptr), DD_ERR_BAD_ARG, "%s: partials and scores are given together or both left out", who);
  DD_REQUIRE(scenes > 0 && n > 0 && k > 0, DD_ERR_BAD_ARG, "%s: non-positive size (scenes %d, n %d, k %d)", who, scenes, n, k);
  DD_REQUIRE(samples >= 1 && samples <= MAX_ROWS, DD_ERR_BAD_ARG, "%s: samples = %d is outside 1 .. %d", who, samples, MAX_ROWS);
  DD_REQUIRE(k % 4 == 0, DD_ERR_UNSUPPORTED, "%s: K = %d must be a multiple of 4", who, k);
  const int nblk = (n + BLOCK - 1) / BLOCK, ntiles = (k + KT - 1) / KT;
  // one workgroup walks the whole contraction, which is what dd_linear_fwd does up to here too: the logits are then the same bits
  DD_REQUIRE(k <= 8 * KT && pick_split(nblk, ntiles) == 1, DD_ERR_UNSUPPORTED,
             "%s: dd_linear_fwd splits K = %d over workgroups (no split up to K = %d)", who, k, 8 * KT);
  const long total = (long)scenes * n;
  DD_REQUIRE(total < (1L << 31), DD_ERR_UNSUPPORTED, "%s: [%d,%d] is too large (scenes * n must stay below 2^31)", who, scenes, n);
  DD_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)mean | (uintptr_t)entropy | (uintptr_t)mi | (uintptr_t)var) & 15) == 0, DD_ERR_BAD_ARG,
             "%s: x, w and the maps must be 16-byte aligned", who);
  DD_REQUIRE(!bias || ((uintptr_t)bias & 3) == 0, DD_ERR_BAD_ARG, "%s: bias must be 4-byte aligned", who);
  DD_REQUIRE((((uintptr_t)partials | (uintptr_t)scores) & 7) == 0, DD_ERR_BAD_ARG, "%s: partials and scores must be 8-byte aligned", who);
  const Span in[3] = {{x, (long)scenes * samples * k * 4, "x"}, {w, (long)n * k * 4, "w"}, {bias, (long)n * 4, "bias"}};
  const Span out[6] = {{mean, total * 4, "mean"},   {entropy, total * 4, "entropy"},
                       {mi, total * 4, "mi"},       {var, total * 4, "var"},
                       {partials, (long)nblk * scenes * 3 * 8, "partials"}, {scores, (long)scenes * 3 * 8, "scores"}};
  for (int i = 0; i < 6; ++i) {
    if (!out[i].p) continue;
    for (int j = 0; j < 3; ++j)
      DD_REQUIRE(!in[j].p || !overlaps(out[i].p, out[i].bytes, in[j].p, in[j].bytes), DD_ERR_BAD_ARG, "%s: %s overlaps the input %s", who,
                 out[i].name, in[j].name);
    for (int j = i + 1; j < 6; ++j)
      DD_REQUIRE(!out[j].p || !overlaps(out[i].p, out[i].bytes, out[j].p, out[j].bytes), DD_ERR_BAD_ARG, "%s: %s overlaps the output %s", who,
                 out[i].name, out[j].name);
  }
  hipStream_t st = (hipStream_t)stream;
  const float inv = (float)(1.0 / samples);
  const int per = MAX_ROWS / samples;      // scenes of a launch
  const dim3 grid(nblk, 1);
  for (int b0 = 0; b0 < scenes; b0 += per) {
    const int nb = min(per, scenes - b0);
    const float* xc = x + (long)b0 * samples * k;
    const long at = (long)b0 * n;
    float *mc = mean ? mean + at : nullptr, *ec = entropy ? entropy + at : nullptr, *ic = mi ? mi + at : nullptr, *vc = var ? var + at : nullptr;
    double* pc = partials ? partials + (long)b0 * 3 : nullptr;
    if (pick_mt(nb * samples) == 1)
      hipLaunchKernelGGL((head_uncert_kernel<1>), grid, dim3(256), 0, st, xc, w, bias, mc, ec, ic, vc, pc, nb, samples, inv, n, k, scenes);
    else
      hipLaunchKernelGGL((head_uncert_kernel<2>), grid, dim3(256), 0, st, xc, w, bias, mc, ec, ic, vc, pc, nb, samples, inv, n, k, scenes);
    DD_LAUNCH_CHECK(who);
  }
  if (scores) {
    hipLaunchKernelGGL(head_uncert_finish, dim3(scenes), dim3(256), 0, st, (const double*)partials, scores, nblk, scenes, (double)n);
    DD_LAUNCH_CHECK(who);
  }
  return 0;
}

}  // extern "C"
