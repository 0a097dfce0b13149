// Global gradient norm for clipping (torch.nn.utils.clip_grad_norm_, norm type 2) without a host round trip and without the gradient
// tensors the rank-B optimizer pass never writes.
//
//   dd_sqnorm / dd_sqnorm_multi   sum g_i^2 over materialised fp32 gradients (one big buffer / a table of small ones)
//   dd_rankb_sqnorm               ||dY^T X||_F^2 (+ ||colsum dY||^2) of a Linear layer from its factors: with Gx = X X^T and Gy = dY dY^T
//                                 (rows x rows each), ||dY^T X||_F^2 = sum_ab Gy_ab Gx_ab and ||db||^2 = sum_ab Gy_ab
//   dd_clip_scale                 the squared norms -> {grad_scale * coef, norm, coef}: what the *_dev optimizer entry points read
//
// Everything is accumulated in fp64: the square of an fp32, and the product of two, is exact there, so the only rounding is that of
// the fp64 sums.  (In fp32 a Gram matrix of a batch whose per-row gradients cancel loses the answer: 24 % error in ||dW||^2 at a
// conditioning of 1e7.)  Every reduction is two-stage and in a fixed order -- per-workgroup fp64 partials in the caller's workspace, a
// single workgroup adds them (the idiom of loss_final_kernel, dense.hip): no atomics, the same bits on every run.
#include <math.h>

#include "dd_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kSqBlocks = DD_NUM_CU * 4;      // workgroups of dd_sqnorm at most (partials: 8 KB)
constexpr int kMultiPerBlock = 1024;          // elements a workgroup of dd_sqnorm_multi takes (4 per thread)
constexpr int kGramBlocks = DD_NUM_CU;        // workgroups of a Gram launch at most (each writes up to 20 KB of partials)
constexpr int kGramStepsPerWave = 8;          // 64-column steps a wave takes at least before another workgroup is worth its partial

// the workgroup's sum of s in a fixed order (tree over 256 threads); valid in thread 0
__device__ __forceinline__ double block_sum_f64(double s, double* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ partial) {
  __shared__ double red[256];
  const long n4 = n / 4;
  double s = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 v = __builtin_nontemporal_load((const f32x4*)g + i);
#pragma unroll
    for (int c = 0; c < 4; ++c) s = fma((double)v[c], (double)v[c], s);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
    const double t = (double)g[4 * n4 + threadIdx.x];
    s = fma(t, t, s);
  }
  const double tot = block_sum_f64(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// The small tensors of a model in one launch, as adam_multi_kernel (dd_adam.h): block b works on tensor t with first[t] <= b < first[t+1].
constexpr int SQ_MULTI_MAX = 48;
struct SqTable {
  const float* g[SQ_MULTI_MAX];
  int n[SQ_MULTI_MAX];
  int first[SQ_MULTI_MAX + 1];
  int count;
};
__global__ __launch_bounds__(256) void sqnorm_multi_kernel(SqTable tab, double* __restrict__ partial) {
  __shared__ double red[256];
  const int t = dd_table_entry(tab.first, tab.count);
  const float* __restrict__ g = tab.g[t];
  const int base = ((int)blockIdx.x - tab.first[t]) * kMultiPerBlock + threadIdx.x;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kMultiPerBlock / 256; ++j) {
    const int i = base + 256 * j;
    const double v = i < tab.n[t] ? (double)g[i] : 0.0;
    s = fma(v, v, s);
  }
  const double tot = block_sum_f64(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// out[0] = sum of the partials, thread-strided then the tree: one order whatever the grid was
__global__ __launch_bounds__(256) void sqnorm_final_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
  const double tot = block_sum_f64(s, red);
  if (threadIdx.x == 0) out[0] = tot;
}

// ---- Gram matrix of the rows of src [rows][cols] in fp64 on the matrix cores -----------------------------------------------------------
// v_mfma_f64_16x16x4_f64: D(16x16) += A(16x4) B(4x16), lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], four
// fp64 results per lane.  With NB = ceil(rows / 16) row blocks the Gram matrix is NB (NB + 1) / 2 blocks bi <= bj (it is symmetric:
// the contraction counts a block bi < bj twice); block (bi, bj) takes A from row block bi and B from row block bj of the SAME
// registers.  A lane loads 16 bytes src[16 b + (l & 15)][c0 + 4 (l >> 4) .. + 3] per row block and 16 columns: element e of the four
// feeds MFMA e, whose contraction set is then {c0 + 4 q + e} -- any assignment of columns to slots is as good as another for a sum over
// all columns, as long as A and B agree, and they are the same register.  WHERE an element of a block lands (the f64 C/D map differs
// from the f32 forms') never matters here: both Gram matrices come out of this kernel in the same order, and the contraction is
// elementwise.
// Columns are split over waves in steps of 64 (dd_range); the four waves of a workgroup add their accumulators in LDS one after the
// other (fixed order) and the workgroup writes ONE partial: [block][register][lane] fp64.
constexpr int gram_blocks(int nb) { return nb * (nb + 1) / 2; }

template <int NB>
__global__ __launch_bounds__(256) void gram_partial_kernel(const float* __restrict__ src, int rows, int cols, double* __restrict__ partial) {
  constexpr int NBLK = gram_blocks(NB);
  __shared__ double sum[NBLK * 256];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  long step, end;
  dd_range(((long)cols + 63) / 64, (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4, step, end);
  f64x4 acc[NBLK];
#pragma unroll
  for (int i = 0; i < NBLK; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (; step < end; ++step) {
    f32x4 v[4][NB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int col = (int)step * 64 + 16 * u + 4 * q;      // cols % 4 == 0: a 16-byte group is all in or all out
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int row = 16 * b + r;
        const bool ok = col < cols && row < rows;
        const f32x4 ld = *(const f32x4*)(src + (ok ? (long)row * cols + col : 0));
        v[u][b] = ok ? ld : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double d[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) d[b] = (double)v[u][b][e];
        int blk = 0;
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) {
#pragma unroll
          for (int bj = bi; bj < NB; ++bj, ++blk) acc[blk] = __builtin_amdgcn_mfma_f64_16x16x4f64(d[bi], d[bj], acc[blk], 0, 0, 0);
        }
      }
    }
  }
  for (int w = 0; w < 4; ++w) {      // wave 0 writes, waves 1..3 add: ((w0 + w1) + w2) + w3
    if (wave == w) {
#pragma unroll
      for (int blk = 0; blk < NBLK; ++blk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double* p = sum + (blk * 4 + i) * 64 + lane;
          *p = (w == 0 ? 0.0 : *p) + acc[blk][i];
        }
      }
    }
    __syncthreads();
  }
  double* out = partial + (long)blockIdx.x * (NBLK * 256);
  for (int i = threadIdx.x; i < NBLK * 256; i += 256) out[i] = sum[i];
}

// The last stage: add the workgroups' partials of both Gram matrices in index order, contract them, write the squared norm.
// gx / gy: [nbx | nby][nelem] fp64; element e belongs to block e / 256, which counts twice when it is off the diagonal.
__global__ __launch_bounds__(256) void gram_contract_kernel(const double* __restrict__ gx, int nbx, const double* __restrict__ gy, int nby,
                                                            int nb, int with_bias, double* __restrict__ out) {
  __shared__ double red[256];
  const int nelem = gram_blocks(nb) * 256;
  double s = 0.0;
  int bi = 0, bj = 0;
  for (int e = threadIdx.x; e < nelem; e += 256) {      // e / 256 walks the blocks (bi, bj), bj fastest from bi
    double x = 0.0, y = 0.0;
    for (int w = 0; w < nbx; ++w) x += gx[(long)w * nelem + e];
    for (int w = 0; w < nby; ++w) y += gy[(long)w * nelem + e];
    const double weight = bi == bj ? 1.0 : 2.0;
    double t = x * y;
    if (with_bias) t += y;
    s = fma(weight, t, s);
    if (++bj == nb) { ++bi; bj = bi; }
  }
  const double tot = block_sum_f64(s, red);
  if (threadIdx.x == 0) out[0] = tot;
}

// One wave: the slots' sum in index order, the norm Adam will see, torch.nn.utils.clip_grad_norm_'s coefficient.
__global__ __launch_bounds__(64) void clip_scale_kernel(const double* __restrict__ sq, int count, float max_norm, float grad_scale,
                                                        float* __restrict__ out3) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < count; ++i) s += sq[i];
  const double norm = (double)grad_scale * sqrt(s);
  double coef = 1.0;
  if (max_norm > 0.f) {
    const double c = (double)max_norm / (norm + 1e-6);
    coef = c > 1.0 ? 1.0 : c;      // torch's clamp(max = 1): a NaN stays a NaN
  }
  out3[0] = (float)((double)grad_scale * coef);
  out3[1] = (float)norm;
  out3[2] = (float)coef;
}

int sqnorm_grid(int64_t n) { return (int)min((n / 4 + 255) / 256 + 1, (int64_t)kSqBlocks); }

int gram_grid(int cols) {
  const long steps = ((long)cols + 63) / 64;
  return (int)max(1L, min((long)kGramBlocks, (steps + 4 * kGramStepsPerWave - 1) / (4 * kGramStepsPerWave)));
}

int64_t gram_partial_bytes(int rows, int cols) {
  const int nb = (rows + 15) / 16;
  return (int64_t)gram_grid(cols) * gram_blocks(nb) * 256 * (int64_t)sizeof(double);
}

void gram_launch(const float* src, int rows, int cols, double* partial, int grid, hipStream_t st) {
  switch ((rows + 15) / 16) {
    case 1: hipLaunchKernelGGL(gram_partial_kernel<1>, dim3(grid), dim3(256), 0, st, src, rows, cols, partial); break;
    case 2: hipLaunchKernelGGL(gram_partial_kernel<2>, dim3(grid), dim3(256), 0, st, src, rows, cols, partial); break;
    case 3: hipLaunchKernelGGL(gram_partial_kernel<3>, dim3(grid), dim3(256), 0, st, src, rows, cols, partial); break;
    default: hipLaunchKernelGGL(gram_partial_kernel<4>, dim3(grid), dim3(256), 0, st, src, rows, cols, partial); break;
  }
}

int64_t multi_blocks(const dd_adam_tensor* tensors, int32_t count) {
  int64_t blocks = 0;
  for (int32_t i = 0; i < count; ++i) {
    if (!tensors[i].g || tensors[i].n <= 0 || tensors[i].n >= (1 << 30)) return -1;
    blocks += (tensors[i].n + kMultiPerBlock - 1) / kMultiPerBlock;
  }
  return blocks;
}

}  // namespace

extern "C" {

int64_t dd_sqnorm_workspace_bytes(int64_t n) {
  if (n <= 0) {
    dd_fail(DD_ERR_BAD_ARG, "sqnorm_workspace_bytes: n = %ld", (long)n);
    return -1;
  }
  return (int64_t)sqnorm_grid(n) * (int64_t)sizeof(double);
}

int dd_sqnorm(const float* g, int64_t n, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  DD_REQUIRE(g && out && workspace && n > 0, DD_ERR_BAD_ARG, "sqnorm: bad argument");
  DD_REQUIRE(((uintptr_t)g % 16 | (uintptr_t)out % 8 | (uintptr_t)workspace % 8) == 0, DD_ERR_BAD_ARG,
             "sqnorm: g must be 16-byte, out and workspace 8-byte aligned");
  const int grid = sqnorm_grid(n);
  DD_REQUIRE(workspace_bytes >= (int64_t)grid * (int64_t)sizeof(double), DD_ERR_WORKSPACE, "sqnorm: workspace too small");
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, (long)n, (double*)workspace);
  DD_LAUNCH_CHECK("sqnorm");
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, grid, out);
  DD_LAUNCH_CHECK("sqnorm final");
  return 0;
}

int64_t dd_sqnorm_multi_workspace_bytes(const dd_adam_tensor* tensors, int32_t count) {
  if (!tensors || count <= 0) {
    dd_fail(DD_ERR_BAD_ARG, "sqnorm_multi_workspace_bytes: bad argument");
    return -1;
  }
  const int64_t blocks = multi_blocks(tensors, count);
  if (blocks < 0 || blocks >= ((int64_t)1 << 31)) {
    dd_fail(DD_ERR_BAD_ARG, "sqnorm_multi_workspace_bytes: a tensor with a NULL gradient or a bad size");
    return -1;
  }
  return blocks * (int64_t)sizeof(double);
}

int dd_sqnorm_multi(const dd_adam_tensor* tensors, int32_t count, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  DD_REQUIRE(tensors && count > 0 && out && workspace, DD_ERR_BAD_ARG, "sqnorm_multi: bad argument");
  DD_REQUIRE(((uintptr_t)out % 8 | (uintptr_t)workspace % 8) == 0, DD_ERR_BAD_ARG, "sqnorm_multi: out and workspace must be 8-byte aligned");
  const int64_t total = multi_blocks(tensors, count);
  DD_REQUIRE(total >= 0 && total < ((int64_t)1 << 31), DD_ERR_BAD_ARG, "sqnorm_multi: a tensor with a NULL gradient or a bad size");
  DD_REQUIRE(workspace_bytes >= total * (int64_t)sizeof(double), DD_ERR_WORKSPACE, "sqnorm_multi: workspace too small");
  int done = 0;      // partials written so far: chunk after chunk, so the final sum runs over the tensors in table order
  for (int32_t base = 0; base < count; base += SQ_MULTI_MAX) {
    SqTable tab;
    tab.count = min(SQ_MULTI_MAX, count - base);
    int blocks = 0;
    for (int i = 0; i < tab.count; ++i) {
      const dd_adam_tensor& t = tensors[base + i];
      tab.g[i] = t.g;
      tab.n[i] = (int)t.n;
      tab.first[i] = blocks;
      blocks += (int)((t.n + kMultiPerBlock - 1) / kMultiPerBlock);
    }
    tab.first[tab.count] = blocks;
    hipLaunchKernelGGL(sqnorm_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tab, (double*)workspace + done);
    DD_LAUNCH_CHECK("sqnorm_multi");
    done += blocks;
  }
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, done, out);
  DD_LAUNCH_CHECK("sqnorm_multi final");
  return 0;
}

int64_t dd_rankb_sqnorm_workspace_bytes(int32_t rows, int32_t n, int32_t k) {
  if (rows <= 0 || n <= 0 || k <= 0 || rows > 64) {
    dd_fail(rows > 64 ? DD_ERR_UNSUPPORTED : DD_ERR_BAD_ARG, "rankb_sqnorm_workspace_bytes: rows = %d, n = %d, k = %d", rows, n, k);
    return -1;
  }
  return gram_partial_bytes(rows, k) + gram_partial_bytes(rows, n);
}

int dd_rankb_sqnorm(const float* dy, const float* x, int32_t rows, int32_t n, int32_t k, int32_t with_bias, double* out, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  DD_REQUIRE(dy && x && out && workspace, DD_ERR_BAD_ARG, "rankb_sqnorm: bad argument");
  DD_REQUIRE(rows > 0 && n > 0 && k > 0, DD_ERR_BAD_ARG, "rankb_sqnorm: non-positive size");
  DD_REQUIRE(rows <= 64, DD_ERR_UNSUPPORTED, "rankb_sqnorm: %d batch rows > 64", rows);
  DD_REQUIRE(k % 4 == 0 && n % 4 == 0, DD_ERR_UNSUPPORTED, "rankb_sqnorm: N = %d and K = %d must be multiples of 4", n, k);
  DD_REQUIRE(((uintptr_t)x % 16 | (uintptr_t)dy % 16 | (uintptr_t)out % 8 | (uintptr_t)workspace % 8) == 0, DD_ERR_BAD_ARG,
             "rankb_sqnorm: factors must be 16-byte, out and workspace 8-byte aligned");
  DD_REQUIRE((int64_t)(rows + 4) * n < ((int64_t)1 << 29) && (int64_t)(rows + 4) * k < ((int64_t)1 << 29), DD_ERR_UNSUPPORTED,
             "rankb_sqnorm: factors of 2 GB or more");
  const int64_t xbytes = gram_partial_bytes(rows, k), ybytes = gram_partial_bytes(rows, n);
  DD_REQUIRE(workspace_bytes >= xbytes + ybytes, DD_ERR_WORKSPACE, "rankb_sqnorm: workspace too small");
  double* gx = (double*)workspace;
  double* gy = (double*)((char*)workspace + xbytes);
  const int gridx = gram_grid(k), gridy = gram_grid(n);
  hipStream_t st = (hipStream_t)stream;
  gram_launch(x, rows, k, gx, gridx, st);
  DD_LAUNCH_CHECK("rankb_sqnorm (x)");
  gram_launch(dy, rows, n, gy, gridy, st);
  DD_LAUNCH_CHECK("rankb_sqnorm (dy)");
  hipLaunchKernelGGL(gram_contract_kernel, dim3(1), dim3(256), 0, st, (const double*)gx, gridx, (const double*)gy, gridy, (rows + 15) / 16,
                     with_bias != 0, out);
  DD_LAUNCH_CHECK("rankb_sqnorm (contract)");
  return 0;
}

int dd_clip_scale(const double* sq, int32_t count, float max_norm, float grad_scale, float* out3, void* stream) {
  DD_REQUIRE(sq && out3 && count > 0, DD_ERR_BAD_ARG, "clip_scale: bad argument");
  DD_REQUIRE(((uintptr_t)sq % 8 | (uintptr_t)out3 % 4) == 0, DD_ERR_BAD_ARG, "clip_scale: misaligned pointer");
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sq, count, max_norm, grad_scale, out3);
  DD_LAUNCH_CHECK("clip_scale");
  return 0;
}

}  // extern "C"
