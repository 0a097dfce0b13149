// The sampled road-map head (include/dd_head_mean.h; csrc/libdd_head_mean.so, a library of its own):
//   dd_head_mean_prob   mean over the S draws of a scene of sigmoid(x W^T + b)   -> fp32 [scenes,n]
//   dd_head_mean_gt     mean > tau                                                -> bytes [scenes,n]; the mean never reaches memory
// One stream over the weight serves up to 64 rows = floor(64 / S) scenes x S draws: the tiles and the contraction are
// linear.hip's (linear_fwd_body, written out again below as fwd_tiles), what dd_linear_fwd and dd_linear_sigmoid_gt run, so the
// accumulators hold their logit bits.
//
// THE GATHER.  An accumulator register holds one column of one row, and the S rows of a scene lie in different registers AND in
// different lanes (row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)): each lane takes the sigmoid of its own elements and the block puts the
// probabilities together as a row-major fp32 tile [rows][128] in the LDS, in the weight's operand tile (32 KB of its 34 KB; the k-loop
// ends on a barrier).  The writes are 32 consecutive dwords per half-wave.  Then lane (tid & 31) of thread row (tid >> 5) owns four
// consecutive columns of the scenes b = tid >> 5, + 8, ...: it reads the S rows of the scene as 16-byte pieces (the 32 lanes of a
// half-wave read one 512-byte row: every 16-lane group of ds_read_b128 on 64 distinct banks) and adds them IN DRAW ORDER, one
// rounded fp32 add each, then one rounded multiply by (float)(1.0 / S).  _prob stores the four means as 16 bytes (n % 4 == 0; else
// element by element); _gt packs the four comparisons into one word of a byte tile [scenes][128] in the activation operand tile and
// stores that tile as dd_linear_sigmoid_gt stores its own (store_byte_tile).  One path for every S, S = 1 included: no
// registers are traded between lanes, no atomics, no scratch.
#include "dd_common.h"

#include "../../include/dd_head_mean.h"

#pragma clang fp contract(off)      // sum + p is ONE rounded add and sum * (1 / S) ONE rounded multiply

namespace {

constexpr int KT = 64;          // k-chunk of the forward kernel
constexpr int WROW = KT + 4;    // LDS row stride in floats: 272 B keeps 16 rows x 16 B on 64 distinct banks

// linear.hip's forward contraction, written out again (the bit-equality tests of tests/test_gpu_head_mean.py hold the two together).
// Y tile [MT*32 rows, 128 columns from n0] += X[M,K] W[N,K]^T over the k-tiles [t0, t1), 256 threads = 4 waves, wave w owns the
// columns [n0 + 32w, +32).  `wl` (128 * WROW floats) and `xl` (MT * 32 * WROW floats) are the caller's LDS operand tiles, 16-byte
// aligned; the loop ends on a barrier, so they are free for the epilogue when this returns.  acc[mt][i] is the element of row
// mt * 32 + dd_acc_row(i, lane), column n0 + 32 * wave + (lane & 31); rows >= M and columns >= N hold exact zeros' products.
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

// The block's MT*32 x 128 byte tile in LDS (row-major, 128 bytes a row) -> Y8 [M, N] as 16-byte stores, a row's 128 bytes from 8 lanes;
// byte by byte where a 16-byte piece could be misaligned or cross the row's end.  The tile has to be complete (a barrier) before this.
template <int MT>
__device__ __forceinline__ void store_byte_tile(const unsigned char* tile, unsigned char* __restrict__ Y8, int M, int N, int n0) {
  const int tid = threadIdx.x;
  const bool vec = N % 16 == 0 && (uintptr_t)Y8 % 16 == 0;      // then a 16-byte piece is aligned, and all inside a row or all outside
  const int c = (tid & 7) * 16;
#pragma unroll
  for (int p = 0; p < MT; ++p) {
    const int m = p * 32 + (tid >> 3);
    if (m >= M || n0 + c >= N) continue;
    unsigned char* dst8 = Y8 + (long)m * N + n0 + c;
    if (vec) {
      *(u32x4*)dst8 = *(const u32x4*)(tile + m * 128 + c);
    } else {
      for (int j = 0; j < min(16, N - n0 - c); ++j) dst8[j] = tile[m * 128 + c + j];
    }
  }
}

// Over how many workgroups dd_linear_fwd splits a contraction of `ntiles` k-tiles when `blocks_other` workgroups cover the output.
// 1 = one workgroup walks the whole contraction: the condition under which a fused kernel holds dd_linear_fwd's own logit bits.
inline int pick_split(int blocks_other, int ntiles) {
  if (ntiles <= 8) return 1;      // a handful of tiles: one block walks them faster than a second launch can add the splits up
  int want = (2 * DD_NUM_CU + blocks_other - 1) / blocks_other;   // aim at ~2 blocks per CU
  want = max(1, min(want, ntiles));
  return min(want, 512);
}

inline int pick_mt(int M) { return M <= 32 ? 1 : (M <= 64 ? 2 : 0); }   // 64 KB of static LDS caps the batch tile at 64 rows
constexpr int MCHUNK = 64;      // more rows than that run once per 64 rows (rows are independent)

constexpr int MAX_ROWS = MCHUNK;      // rows of a launch: floor(64 / S) scenes of S draws

// grid ceil(N / 128); 4 waves.  X: the launch's nb * S rows; out: its nb rows.
template <int MT, bool GT>
__global__ __launch_bounds__(256) void head_mean_kernel(const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                        float tau, void* __restrict__ out, int nb, int S, float inv, int N, int K) {
  __shared__ __attribute__((aligned(16))) float wl[128 * WROW];
  __shared__ __attribute__((aligned(16))) float xl[MT * 32 * WROW];
  static_assert(MT * 32 * 128 <= 128 * WROW, "the probability tile lies in the weight's operand tile");
  static_assert(MT * 32 * 128 <= MT * 32 * WROW * 4, "the byte tile lies in the activation operand tile");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31;
  const int n0 = blockIdx.x * 128;

  f32x16 acc[MT];
  fwd_tiles<MT>(X, Wt, nb * S, N, K, n0, 0, (K + KT - 1) / KT, wl, xl, acc, tid, wave);

  const int n = n0 + wave * 32 + r;
  const float bv = (bias && n < N) ? bias[n] : 0.f;
  float* ptile = wl;      // [MT*32][128]; rows past nb * S and columns past N hold sigmoid(bias) of zeros: finite, never read out
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float sig, l1p;
      dd_sigmoid_softplus(acc[mt][i] + bv, sig, l1p);      // the dense head's one sigmoid; the softplus half is dead code here
      ptile[(mt * 32 + dd_acc_row(i, lane)) * 128 + wave * 32 + r] = sig;
    }
  __syncthreads();

  const int cg = tid & 31, c = 4 * cg;      // this lane's four columns of the tile
  unsigned* btile = (unsigned*)xl;          // GT: [nb][128] bytes, a word = four columns
  for (int b = tid >> 5; b < nb; b += 8) {
    const float* row = ptile + b * S * 128 + c;
    f32x4 sum = *(const f32x4*)row;
    for (int s = 1; s < S; ++s) sum += *(const f32x4*)(row + s * 128);      // draw order
    const f32x4 mean = sum * inv;
    if constexpr (GT) {
      unsigned word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) word |= (mean[j] > tau ? 1u : 0u) << (8 * j);      // a NaN mean is 0
      btile[b * 32 + cg] = word;
    } else {
      float* dst = (float*)out + (long)b * N + n0 + c;
      if (N % 4 == 0) {      // then the four columns are all inside the row or all outside, and 16-byte aligned
        if (n0 + c < N) *(f32x4*)dst = mean;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n0 + c + j < N) dst[j] = mean[j];
      }
    }
  }
  if constexpr (GT) {
    __syncthreads();
    store_byte_tile<MT>((const unsigned char*)btile, (unsigned char*)out, nb, N, n0);
  }
}

bool overlaps(const void* p, long p_bytes, const void* q, long q_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}

template <bool GT>
int launch_mean(const char* who, const float* x, const float* w, const float* bias, float tau, void* out, int scenes, int samples, int n,
                int k, void* stream) {
  DD_REQUIRE(x && w && out, DD_ERR_BAD_ARG, "%s: NULL pointer", who);
  DD_REQUIRE(scenes > 0 && n > 0 && k > 0, DD_ERR_BAD_ARG, "%s: non-positive size (scenes %d, n %d, k %d)", who, scenes, n, k);
  DD_REQUIRE(samples >= 1 && samples <= MAX_ROWS, DD_ERR_BAD_ARG, "%s: samples = %d is outside 1 .. %d", who, samples, MAX_ROWS);
  DD_REQUIRE(k % 4 == 0, DD_ERR_UNSUPPORTED, "%s: K = %d must be a multiple of 4", who, k);
  const int nblk = (n + 127) / 128, ntiles = (k + KT - 1) / KT;
  // one workgroup walks the whole contraction, which is what dd_linear_fwd does up to here too: the logits are then the same bits
  DD_REQUIRE(k <= 8 * KT && pick_split(nblk, ntiles) == 1, DD_ERR_UNSUPPORTED,
             "%s: dd_linear_fwd splits K = %d over workgroups (no split up to K = %d)", who, k, 8 * KT);
  const long total = (long)scenes * n;
  DD_REQUIRE(total < (1L << 31), DD_ERR_UNSUPPORTED, "%s: [%d,%d] is too large (scenes * n must stay below 2^31)", who, scenes, n);
  DD_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) & 15) == 0, DD_ERR_BAD_ARG, "%s: x, w and out must be 16-byte aligned", who);
  DD_REQUIRE(!bias || ((uintptr_t)bias & 3) == 0, DD_ERR_BAD_ARG, "%s: bias must be 4-byte aligned", who);
  const long out_bytes = total * (GT ? 1 : 4);
  DD_REQUIRE(!overlaps(out, out_bytes, x, (long)scenes * samples * k * 4) && !overlaps(out, out_bytes, w, (long)n * k * 4) &&
                 !(bias && overlaps(out, out_bytes, bias, (long)n * 4)),
             DD_ERR_BAD_ARG, "%s: out overlaps an input", who);
  hipStream_t st = (hipStream_t)stream;
  const float inv = (float)(1.0 / samples);
  const int per = MAX_ROWS / samples;      // scenes of a launch
  const dim3 grid(nblk, 1);
  for (int b0 = 0; b0 < scenes; b0 += per) {
    const int nb = min(per, scenes - b0);
    const float* xc = x + (long)b0 * samples * k;
    void* oc = GT ? (void*)((unsigned char*)out + (long)b0 * n) : (void*)((float*)out + (long)b0 * n);
    if (pick_mt(nb * samples) == 1)
      hipLaunchKernelGGL((head_mean_kernel<1, GT>), grid, dim3(256), 0, st, xc, w, bias, tau, oc, nb, samples, inv, n, k);
    else
      hipLaunchKernelGGL((head_mean_kernel<2, GT>), grid, dim3(256), 0, st, xc, w, bias, tau, oc, nb, samples, inv, n, k);
    DD_LAUNCH_CHECK(who);
  }
  return 0;
}

}  // namespace

extern "C" {

int dd_head_mean_prob(const float* x, const float* w, const float* bias, float* out, int32_t scenes, int32_t samples, int32_t n, int32_t k,
                      void* stream) {
  return launch_mean<false>("head_mean_prob", x, w, bias, 0.f, out, scenes, samples, n, k, stream);
}

int dd_head_mean_gt(const float* x, const float* w, const float* bias, float tau, unsigned char* out, int32_t scenes, int32_t samples,
                    int32_t n, int32_t k, void* stream) {
  return launch_mean<true>("head_mean_gt", x, w, bias, tau, out, scenes, samples, n, k, stream);
}

}  // extern "C"
