// Box-level validation on the device: predicted occupancy map -> connected components -> axis-aligned boxes -> pairwise IoU ->
// average threat score (reference src/utils/helper.py:33-83, compute_ats_bounding_boxes / compute_iou).  The inverse direction of
// raster.hip.  None of this touches the matrix cores: the labelling is bound by latency (pointer chasing), the rest by HBM.
//
// a. dd_label_components: 4-connected components of `map > threshold`, as a union-find over pixels.  The output buffer IS the parent
//    array while the kernels run: labels[p] = parent(p) + 1 for a foreground pixel, 0 for background (p = row * W + col inside its
//    sample; nothing ever points across samples).  INVARIANT, kept by every write below: parent(p) <= p and parent(p) is a pixel
//    of p's component.  So every parent chain strictly decreases until it reaches a root (parent(r) == r), a tree's root is its
//    smallest pixel, and once all neighbouring pairs are united the root is the component's FIRST PIXEL IN RASTER ORDER -- the
//    canonical label, independent of scheduling.
//      1. tile_label_kernel: one workgroup per 32x32 tile, union-find in LDS over the tile's pixels (left and upper neighbour of each
//         pixel), then every pixel is written with its tile root (local raster order == global raster order inside a tile).
//      2. border_merge_kernel: one thread per pixel on a tile's left column / top row unites it with its neighbour across the border,
//         with vector atomicMin on the global array.
//      3. flatten_kernel: labels[p] = root(p) + 1.
//    LOOP BOUNDS.  find(): the index strictly decreases, so at most `n` steps (n = pixels in the tile / in the sample); the loops are
//    written `for (it < n)` so that they end even if the invariant were broken.  unite(a, b): every round that does not return
//    replaces (a, b) by two roots that are both smaller than the old max(a, b) (see the function), so at most `n` rounds; written the
//    same way.  No kernel waits for another workgroup: an atomicMin that loses a race returns the winner's value and the loop goes on
//    from there with a strictly smaller pair.  Stale (cached) reads of the parent array are harmless: an old parent is still an
//    ancestor in the same tree with a smaller index.
// b. THE FIT: labels -> boxes.  ONE pipeline (fit_launch<kRegions>, the only list of its launches), two instantiations, four entry points:
//    dd_component_boxes / dd_component_obb (kRegions = false: a. into the workspace, then the fit of those labels) and dd_labelled_boxes /
//    dd_labelled_obb (kRegions = true: the fit of a label image the caller brings, b''.).  The launches: label (a., whose flatten zeroes the
//    roots' records) or region_init; stats: per component pixel count and extents by integer atomics at the root's slot (one set of atomics
//    per horizontal run inside a 64-pixel segment, found with a ballot -- no loop); row count / row scan / in-row scan: a compaction that
//    orders the survivors by label; then emit, or b'.'s four launches.  Integer atomics only, so the result is deterministic.
//    The two instantiations differ in three places and nowhere else: where a run ends (run_length: component_run / region_run), which record
//    is zeroed (the root's / the one at pixel label - 1), and the top row (the root's row / a real maximum of H - 1 - y kept in `top`).
//    kRegions = false touches no `top` array, loads no lab[v - 1] and launches nothing more than it needs.
// b'. fit = oriented: the same components, the same survivors in the same order, but each fitted with an ORIENTED box: the principal
//    axis of its pixel cloud from exact integer second moments, then the extents of the pixel centres along and across that axis.
//    After b.'s labelling, count and ordering launches: slot (the emit structure) gives every survivor its output slot and a zeroed
//    record there; moment (the run structure) adds each run's closed-form sums to the record with 64-bit integer atomics; extent (the
//    run structure again, a SEPARATE launch, so every moment is final) projects the two end pixels of each run -- u and v are monotone
//    along a run -- and folds them in with 64-bit integer max on an order-preserving encoding of the fp64 value; emit writes the
//    corners.  Integer add and integer max only: bit-identical from launch to launch.  Every thread that needs the heading evaluates
//    the one function heading() on the same integers, so all of them agree bit for bit.  No loop in any of the four kernels except the
//    slot kernel's walk along its row (W / 256 rounds, as in emit_boxes_kernel).
// b''. dd_split_components: marker-based splitting of blobs joined by a neck (the rule is stated in include/dd_hotpath.h).
//    erode (LDS, separable minimum) -> a.'s launches on the core map -> grow (g Jacobi rounds between two LDS buffers, one barrier per
//    round, smallest neighbouring label wins) -> a.'s launches on what is left -> merge.  The result is a LABEL IMAGE whose regions are
//    sets of equal labels, label - 1 being SOME pixel of the region (not its first): what b.'s kRegions = true instantiation fits.
//    LOOP BOUNDS: erode 2 r + 1 <= 17 taps, grow g <= 16 rounds of at most 16 pixels per thread.
// c. dd_box_iou_ats: one thread per box pair, fp64, Green's theorem over the boundary of the intersection (fully unrolled: no
//    indexed local array, no scratch), then one workgroup per sample for max over set 1, the five thresholds and the weighted mean.
#include "dd_common.h"

// the IoU's sign tests rely on x*y - z*w being exactly zero for equal products and exactly negated when the operands swap: no FMA
#pragma clang fp contract(off)

namespace {

constexpr int kTile = 32;                 // tile side of the LDS phase
constexpr int kTilePix = kTile * kTile;
constexpr int kThreads = 256;
constexpr int kMaxSide = 8192;            // H, W
constexpr int kMaxBatch = 65535;          // gridDim.z
constexpr int kMaxSet = 4096;             // boxes per sample and set in dd_box_iou_ats
constexpr int kObbMaxSide = 1024;         // H, W in dd_component_obb: N <= 2^20 and Sxx <= N * 1023^2 < 2^40, so N * Sxx < 2^60 fits int64
constexpr int kObbMaxBoxes = kObbMaxSide * kObbMaxSide;      // no sample has more components than pixels
constexpr int kMaxSplit = 8;              // split_px: the erode tile with its halo is (32 + 16)^2 bytes of LDS
constexpr int kMaxGrow = 16;              // grow_iters: two label buffers of (32 + 32)^2 ints = 32 KB of LDS

// ------------------------------------------------------------------------------------------------ a. labelling
__device__ __forceinline__ int lds_parent(const int* par, int x) { return __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// root of x in the tile's forest.  Bound: par[x] < x for every non-root, so x strictly decreases: at most kTilePix steps.
__device__ __forceinline__ int lds_find(const int* par, int x) {
  for (int it = 0; it < kTilePix; ++it) {
    const int p = lds_parent(par, x);
    if (p == x) break;
    x = p;
  }
  return x;
}

// Unite the trees of a and b.  Each round: a, b := their roots; equal -> done; otherwise hang the larger root (call it a) under the
// smaller with atomicMin.  If the old value was a itself the link is made.  If not, another thread hung a under `old` < a in the
// meantime; par[a] is now min(old, b), and uniting old with b restores the connection whichever of the two won.  The new pair
// (old, b) has both members < a = the old maximum, so the maximum strictly decreases: at most kTilePix rounds.
__device__ __forceinline__ void lds_unite(int* par, int a, int b) {
  for (int it = 0; it < kTilePix; ++it) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(kThreads) void tile_label_kernel(const float* __restrict__ maps, float threshold, int* __restrict__ labels,
                                                              int H, int W) {
  __shared__ int par[kTilePix];
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const long base = (long)blockIdx.z * H * W;
  unsigned fg = 0;                                                    // bit k: pixel threadIdx.x + 256 k of the tile is foreground
#pragma unroll
  for (int k = 0; k < kTilePix / kThreads; ++k) {
    const int i = threadIdx.x + kThreads * k;
    const int y = y0 + i / kTile, x = x0 + i % kTile;
    const bool f = y < H && x < W && maps[base + (long)y * W + x] > threshold;      // bounds first: ragged tiles read nothing outside
    fg |= (unsigned)f << k;
    par[i] = f ? i : -1;
  }
  __syncthreads();
  // background entries stay -1 and are never the target of an atomic; foreground entries stay >= 0
#pragma unroll
  for (int k = 0; k < kTilePix / kThreads; ++k) {
    const int i = threadIdx.x + kThreads * k;
    if (!((fg >> k) & 1u)) continue;
    if (i % kTile > 0 && lds_parent(par, i - 1) >= 0) lds_unite(par, i, i - 1);
    if (i >= kTile && lds_parent(par, i - kTile) >= 0) lds_unite(par, i, i - kTile);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTilePix / kThreads; ++k) {
    const int i = threadIdx.x + kThreads * k;
    const int y = y0 + i / kTile, x = x0 + i % kTile;
    if (y >= H || x >= W) continue;
    int v = 0;
    if ((fg >> k) & 1u) {
      const int r = lds_find(par, i);                                 // the tile root: smallest local index == smallest global index
      v = (y0 + r / kTile) * W + x0 + r % kTile + 1;
    }
    labels[base + (long)y * W + x] = v;
  }
}

__device__ __forceinline__ int g_parent(const int* lab, int x) { return __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1; }

// root of x in the sample's forest (lab = the sample's labels, n = H * W).  x strictly decreases: at most n steps.  `halve`
// also hangs x under its grandparent (atomicMin: the entry only ever decreases and stays inside the component -- the invariant).
template <bool kHalve>
__device__ __forceinline__ int g_find(int* lab, int x, int n) {
  for (int it = 0; it < n; ++it) {
    const int p = g_parent(lab, x);
    if (p == x) break;
    if (kHalve) {
      const int gp = g_parent(lab, p);
      if (gp != p) atomicMin(lab + x, gp + 1);
    }
    x = p;
  }
  return x;
}

// lds_unite on the global array; the same argument bounds it by n rounds.
__device__ __forceinline__ void g_unite(int* lab, int a, int b, int n) {
  for (int it = 0; it < n; ++it) {
    a = g_find<true>(lab, a, n);
    b = g_find<true>(lab, b, n);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b + 1) - 1;
    if (old == a) return;
    a = old;
  }
}

// items of one sample: nv vertical borders (columns kTile, 2 kTile, ...) of H pixels each, then nh horizontal borders of W pixels
__global__ __launch_bounds__(kThreads) void border_merge_kernel(int* __restrict__ labels, int H, int W, int nv, int nh) {
  int* lab = labels + (long)blockIdx.y * H * W;
  const int n = H * W;
  int idx = blockIdx.x * kThreads + threadIdx.x;
  int p, q;
  if (idx < nv * H) {
    const int x = (idx / H + 1) * kTile, y = idx % H;                 // x <= nv * kTile <= W - 1
    p = y * W + x;
    q = p - 1;
  } else {
    idx -= nv * H;
    if (idx >= nh * W) return;
    const int y = (idx / W + 1) * kTile, x = idx % W;                 // y <= nh * kTile <= H - 1
    p = y * W + x;
    q = p - W;
  }
  if (g_parent(lab, p) >= 0 && g_parent(lab, q) >= 0) g_unite(lab, p, q, n);
}

struct Stats {        // per component, at its root pixel's slot; all maxima, so zero initialises them
  int count, w1_minus_c0, c1, r1;
};

// labels[p] = root + 1.  In place: a thread that walks through p meanwhile sees the old parent or the root, both ancestors.
__global__ __launch_bounds__(kThreads) void flatten_kernel(int* __restrict__ labels, Stats* __restrict__ stats, int n) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  int* lab = labels + (long)blockIdx.y * n;
  if (g_parent(lab, p) < 0) return;
  const int r = g_find<false>(lab, p, n);
  __hip_atomic_store(lab + p, r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (stats && r == p) stats[(long)blockIdx.y * n + p] = Stats{0, 0, 0, 0};
}

int label_launch(const float* maps, float threshold, int* labels, Stats* stats, int batch, int H, int W, hipStream_t st) {
  const int tx = (W + kTile - 1) / kTile, ty = (H + kTile - 1) / kTile;
  hipLaunchKernelGGL(tile_label_kernel, dim3(tx, ty, batch), dim3(kThreads), 0, st, maps, threshold, labels, H, W);
  DD_LAUNCH_CHECK("label_components tiles");
  const int nv = (W - 1) / kTile, nh = (H - 1) / kTile;
  const long items = (long)nv * H + (long)nh * W;
  if (items > 0) {
    hipLaunchKernelGGL(border_merge_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads), batch), dim3(kThreads), 0, st, labels, H, W,
                       nv, nh);
    DD_LAUNCH_CHECK("label_components borders");
  }
  const int n = H * W;
  hipLaunchKernelGGL(flatten_kernel, dim3((n + kThreads - 1) / kThreads, batch), dim3(kThreads), 0, st, labels, stats, n);
  DD_LAUNCH_CHECK("label_components flatten");
  return 0;
}

long align16(long v) { return (v + 15) & ~15L; }

bool shape_ok(int batch, int H, int W) { return batch >= 1 && batch <= kMaxBatch && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide; }

// ------------------------------------------------------------------------------------------------ b. component boxes
// One wave per 64-pixel segment of a row.  Horizontally adjacent foreground pixels share their label, so a run of set bits in the
// ballot is one component: its first lane adds the run to the root's slot.
// component_run (kRegions = false, dd_label_components' labels): whether a run of foreground begins at this lane, and then its length.  (A bool
// and not "0 when none does", as region_run has it: with that the compiler forms the length before it leaves, for 2-3 more registers.)
__device__ __forceinline__ bool component_run(int v, int lane, int& len) {
  const unsigned long long mask = __ballot(v != 0);
  if (v == 0 || (lane > 0 && ((mask >> (lane - 1)) & 1ull))) return false;
  const unsigned long long inv = ~(mask >> lane);                     // lowest zero bit = end of the run; none: the run fills the segment
  len = inv ? __ffsll((long long)inv) - 1 : 64;
  return true;
}

// region_run (kRegions = true, a label image, b''.): the length of the run of EQUAL labels that begins at this lane, 0 when none does -- a run
// also ends where the label changes.  A label outside [1, n], or one whose pixel label - 1 does not carry it, belongs to no region and
// starts no run, so no record outside the sample's n slots is ever touched, whatever the image holds.  v: sanitised in place.
__device__ __forceinline__ int region_run(const int* lab, int n, int& v, int lane) {
  if (v < 0 || v > n) v = 0;
  const unsigned long long mask = __ballot(v != 0);
  const int left = __shfl_up(v, 1);
  const bool start = v != 0 && (lane == 0 || left != v);
  const unsigned long long brk = __ballot(start) | ~mask;             // where a run cannot go on
  if (!start || lab[v - 1] != v) return 0;
  const unsigned long long rest = (brk >> lane) >> 1;                 // lanes after this one
  return rest ? __ffsll((long long)rest) : 64 - lane;
}

// whether a run begins at this lane of the wave's 64-pixel segment, and then its length; lab = the sample's labels, n = H * W
template <bool kRegions>
__device__ __forceinline__ bool run_length(const int* lab, int n, int& v, int lane, int& len) {
  if constexpr (kRegions) return (len = region_run(lab, n, v, lane)) != 0;
  else return component_run(v, lane, len);
}

// `top` exists for a label image only (null otherwise): label - 1 need not lie in the region's first row
template <bool kRegions>
__global__ __launch_bounds__(kThreads) void run_stats_kernel(const int* __restrict__ labels, Stats* __restrict__ stats, int H, int W, int* __restrict__ top) {
  const int lane = threadIdx.x, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
  const long base = (long)blockIdx.z * H * W;
  int v = (x < W && y < H) ? labels[base + (long)y * W + x] : 0;
  int len;
  if (!run_length<kRegions>(labels + base, H * W, v, lane, len)) return;
  Stats* s = stats + base + (v - 1);
  atomicAdd(&s->count, len);
  atomicMax(&s->w1_minus_c0, W - 1 - x);
  atomicMax(&s->c1, x + len - 1);
  atomicMax(&s->r1, y);
  if constexpr (kRegions) atomicMax(top + base + (v - 1), H - 1 - y);
}

// flatten_kernel's second duty for a label image: the records of the pixels that name a region (labels[p] == p + 1) start at zero
__global__ __launch_bounds__(kThreads) void region_init_kernel(const int* __restrict__ labels, Stats* __restrict__ stats, int* __restrict__ top, int n) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  const long i = (long)blockIdx.y * n + p;
  if (labels[i] != p + 1) return;
  stats[i] = Stats{0, 0, 0, 0};
  top[i] = 0;
}

// exclusive prefix sum of v over the workgroup's 256 threads; total = the sum.  wsum: 4 ints of LDS.
__device__ __forceinline__ int block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();                                                    // wsum may still be read from the previous call
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    const int t = wsum[k];
    if (k < w) off += t;
    total += t;
  }
  return off + inc - v;
}

__device__ __forceinline__ bool survivor(const int* lab, const Stats* st, int p, int min_pixels) {
  return lab[p] == p + 1 && st[p].count >= min_pixels;
}

__global__ __launch_bounds__(kThreads) void row_count_kernel(const int* __restrict__ labels, const Stats* __restrict__ stats, int* __restrict__ rowcnt,
                                                             int H, int W, int min_pixels) {
  __shared__ int wsum[kThreads / 64];
  const int y = blockIdx.x, s = blockIdx.y;
  const long base = (long)s * H * W;
  int c = 0;
  for (int x = threadIdx.x; x < W; x += kThreads) c += survivor(labels + base, stats + base, y * W + x, min_pixels);
  int total;
  block_scan(c, wsum, total);
  if (threadIdx.x == 0) rowcnt[s * H + y] = total;
}

__global__ __launch_bounds__(kThreads) void row_scan_kernel(const int* __restrict__ rowcnt, int* __restrict__ rowbase, int* __restrict__ counts, int H) {
  __shared__ int wsum[kThreads / 64];
  const int s = blockIdx.x;
  int carry = 0;
  for (int y0 = 0; y0 < H; y0 += kThreads) {                          // uniform trip count: the scan's barriers are reached by all
    const int y = y0 + threadIdx.x;
    const int v = y < H ? rowcnt[s * H + y] : 0;
    int total;
    const int ex = block_scan(v, wsum, total);
    if (y < H) rowbase[s * H + y] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) counts[s] = carry;                            // uncapped
}

// kRegions: the pixel label - 1 that names a region need not lie in its top row, so r0 comes from `top` (null otherwise), a real maximum
// over the region's rows.  A component's root is its first pixel in raster order: its row is r0.  (While the two were separate kernels the
// compiler placed one scalar OR of the kRegions = false one differently from what it does for this template; nothing else differs.)
template <bool kRegions>
__global__ __launch_bounds__(kThreads) void emit_boxes_kernel(const int* __restrict__ labels, const Stats* __restrict__ stats, const int* __restrict__ rowcnt,
                                                              const int* __restrict__ rowbase, float* __restrict__ boxes, int H, int W,
                                                              int min_pixels, int max_boxes, const int* __restrict__ top) {
  __shared__ int wsum[kThreads / 64];
  const int y = blockIdx.x, s = blockIdx.y;
  if (rowcnt[s * H + y] == 0) return;                                 // uniform
  const long base = (long)s * H * W;
  int carry = rowbase[s * H + y];
  for (int x0 = 0; x0 < W; x0 += kThreads) {
    const int x = x0 + threadIdx.x;
    const bool f = x < W && survivor(labels + base, stats + base, y * W + x, min_pixels);
    int total;
    const int slot = carry + block_scan(f, wsum, total);
    carry += total;
    if (f && slot < max_boxes) {                                      // the only store: slot in [0, max_boxes)
      const Stats st = stats[base + y * W + x];
      int r0 = y;
      if constexpr (kRegions) r0 = H - 1 - top[base + y * W + x];
      const int c0 = W - 1 - st.w1_minus_c0, c1 = st.c1, r1 = st.r1;
      const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;        // exact: multiples of 0.5 far below 2^23
      const float xmin = ((float)c0 - hw) / 10.f, xmax = ((float)(c1 + 1) - hw) / 10.f;
      const float ymin = (hh - (float)(r1 + 1)) / 10.f, ymax = (hh - (float)r0) / 10.f;
      float* o = boxes + ((long)s * max_boxes + slot) * 8;
      o[0] = xmax; o[1] = xmax; o[2] = xmin; o[3] = xmin;
      o[4] = ymax; o[5] = ymin; o[6] = ymax; o[7] = ymin;
    }
  }
}

// ------------------------------------------------------------------------------------------------ b'. oriented boxes
struct Obb {          // per survivor, at its output slot; zero initialises all of it (the four extents are maxima of codes that are never 0)
  long long n, sx, sy, sxx, sxy, syy;
  unsigned long long u1, neg_u0, v1, neg_v0;      // code(max u), code(max -u), code(max v), code(max -v)
};

// fp64 -> uint64, order-preserving (a < b  <=>  code(a) < code(b), -0 below +0); code(-inf) = 2^52 - 1 > 0 is the smallest code
__device__ __forceinline__ unsigned long long code(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

__device__ __forceinline__ double decode(unsigned long long e) {
  return __longlong_as_double((long long)((e >> 63) ? e & 0x7fffffffffffffffull : ~e));
}

// the major axis of the pixel cloud: theta = atan2(2 mxy, mxx - myy) / 2 in (-pi/2, pi/2], from N^2 times the central second moments,
// which are exact in int64 for sides up to kObbMaxSide.  A cloud without a direction (mxy == 0, mxx == myy) gives atan2(0, 0) = 0.
__device__ __forceinline__ void heading(const Obb& m, double& c, double& s) {
  const long long mxx = m.n * m.sxx - m.sx * m.sx, myy = m.n * m.syy - m.sy * m.sy, mxy = m.n * m.sxy - m.sx * m.sy;
  const double theta = 0.5 * atan2(2.0 * (double)mxy, (double)(mxx - myy));
  c = cos(theta);
  s = sin(theta);
}

// The slot of every survivor, in label order (emit_boxes_kernel's walk).  The extents of b. are not used on this path: the survivor's
// c1 field is overwritten with its slot (uncapped), and the record of a slot below max_boxes is zeroed except for the pixel count.
__global__ __launch_bounds__(kThreads) void obb_slot_kernel(const int* __restrict__ labels, Stats* __restrict__ stats, const int* __restrict__ rowcnt,
                                                            const int* __restrict__ rowbase, Obb* __restrict__ recs, int H, int W, int min_pixels,
                                                            int max_boxes) {
  __shared__ int wsum[kThreads / 64];
  const int y = blockIdx.x, s = blockIdx.y;
  if (rowcnt[s * H + y] == 0) return;                                 // uniform
  const long base = (long)s * H * W;
  int carry = rowbase[s * H + y];
  for (int x0 = 0; x0 < W; x0 += kThreads) {                          // ceil(W / 256) rounds, uniform: the scan's barriers are reached by all
    const int x = x0 + threadIdx.x;
    const bool f = x < W && survivor(labels + base, stats + base, y * W + x, min_pixels);
    int total;
    const int slot = carry + block_scan(f, wsum, total);
    carry += total;
    if (f) {
      Stats* st = stats + base + y * W + x;
      st->c1 = slot;
      if (slot < max_boxes) recs[(long)s * max_boxes + slot] = Obb{st->count, 0, 0, 0, 0, 0, 0ull, 0ull, 0ull, 0ull};      // slot in [0, max_boxes)
    }
  }
}

// the record of the component with label v, or null when it is no survivor or lies past the cap
__device__ __forceinline__ Obb* obb_record(const Stats* __restrict__ stats, Obb* __restrict__ recs, long base, int sample, int v, int min_pixels,
                                           int max_boxes) {
  const Stats st = stats[base + (v - 1)];
  if (st.count < min_pixels || st.c1 >= max_boxes) return nullptr;   // c1 = the slot, >= 0, written by obb_slot_kernel for every survivor
  return recs + (long)sample * max_boxes + st.c1;
}

// run_stats_kernel's structure.  The run [x, x + len) of row y adds sum 1, X, Y, X^2, X Y, Y^2 in closed form (len <= 64: no overflow).
template <bool kRegions>
__global__ __launch_bounds__(kThreads) void obb_moment_kernel(const int* __restrict__ labels, const Stats* __restrict__ stats, Obb* __restrict__ recs,
                                                              int H, int W, int min_pixels, int max_boxes) {
  const int lane = threadIdx.x, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
  const long base = (long)blockIdx.z * H * W;
  int v = (x < W && y < H) ? labels[base + (long)y * W + x] : 0;
  int run;
  if (!run_length<kRegions>(labels + base, H * W, v, lane, run)) return;
  const long long len = run;
  Obb* r = obb_record(stats, recs, base, blockIdx.z, v, min_pixels, max_boxes);
  if (!r) return;
  const long long tri = len * (len - 1) / 2, sx = len * x + tri;
  const long long sxx = len * x * x + 2 * x * tri + (len - 1) * len * (2 * len - 1) / 6;
  atomicAdd((unsigned long long*)&r->sx, (unsigned long long)sx);
  atomicAdd((unsigned long long*)&r->sy, (unsigned long long)(len * y));
  atomicAdd((unsigned long long*)&r->sxx, (unsigned long long)sxx);
  atomicAdd((unsigned long long*)&r->sxy, (unsigned long long)(sx * y));
  atomicAdd((unsigned long long*)&r->syy, (unsigned long long)(len * y * y));
}

// After the moment launch.  u = (X + .5) c + (Y + .5) s and v = -(X + .5) s + (Y + .5) c are monotone in X along a row (a rounded product
// and a rounded sum are monotone in their operand), so the run's extremes are at its two end pixels.
template <bool kRegions>
__global__ __launch_bounds__(kThreads) void obb_extent_kernel(const int* __restrict__ labels, const Stats* __restrict__ stats, Obb* __restrict__ recs,
                                                              int H, int W, int min_pixels, int max_boxes) {
  const int lane = threadIdx.x, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
  const long base = (long)blockIdx.z * H * W;
  int v = (x < W && y < H) ? labels[base + (long)y * W + x] : 0;
  int len;
  if (!run_length<kRegions>(labels + base, H * W, v, lane, len)) return;
  Obb* r = obb_record(stats, recs, base, blockIdx.z, v, min_pixels, max_boxes);
  if (!r) return;
  double c, s;
  heading(*r, c, s);
  const double xa = (double)x + 0.5, xb = (double)(x + len - 1) + 0.5, yc = (double)y + 0.5;
  const double ua = xa * c + yc * s, ub = xb * c + yc * s, va = -xa * s + yc * c, vb = -xb * s + yc * c;
  atomicMax(&r->u1, code(fmax(ua, ub)));
  atomicMax(&r->neg_u0, code(-fmin(ua, ub)));
  atomicMax(&r->v1, code(fmax(va, vb)));
  atomicMax(&r->neg_v0, code(-fmin(va, vb)));
}

// one thread per stored box: extents moved outwards by pad (|c| + |s|), the ring (u1,v1), (u1,v0), (u0,v0), (u0,v1) rotated back to
// pixel coordinates and mapped to metres in fp64, ONE rounding to fp32.  The ring goes to columns 0, 1, 3, 2.
__global__ __launch_bounds__(kThreads) void obb_emit_kernel(const Obb* __restrict__ recs, const int* __restrict__ counts, float pad_px,
                                                            float* __restrict__ boxes, long long* __restrict__ moments, int H, int W, int max_boxes) {
  const int slot = blockIdx.x * kThreads + threadIdx.x, smp = blockIdx.y;
  if (slot >= max_boxes || slot >= counts[smp]) return;               // the only stores: slot in [0, max_boxes)
  const long i = (long)smp * max_boxes + slot;
  const Obb m = recs[i];
  double c, s;
  heading(m, c, s);
  const double pad = (double)pad_px * (fabs(c) + fabs(s));
  const double u0 = -decode(m.neg_u0) - pad, u1 = decode(m.u1) + pad, v0 = -decode(m.neg_v0) - pad, v1 = decode(m.v1) + pad;
  const double hw = 0.5 * (double)W, hh = 0.5 * (double)H;
  const double ru[4] = {u1, u1, u0, u0}, rv[4] = {v1, v0, v0, v1};
  const int col[4] = {0, 1, 3, 2};
  float* o = boxes + i * 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double X = ru[k] * c - rv[k] * s, Y = ru[k] * s + rv[k] * c;
    o[col[k]] = (float)((X - hw) / 10.0);
    o[4 + col[k]] = (float)((hh - Y) / 10.0);
  }
  if (moments) {
    long long* q = moments + i * 6;
    q[0] = m.n; q[1] = m.sx; q[2] = m.sy; q[3] = m.sxx; q[4] = m.sxy; q[5] = m.syy;
  }
}

bool obb_shape_ok(int batch, int H, int W, int max_boxes) {
  return batch >= 1 && batch <= kMaxBatch && H >= 1 && W >= 1 && H <= kObbMaxSide && W <= kObbMaxSide && max_boxes >= 1 && max_boxes <= kObbMaxBoxes;
}

// ------------------------------------------------------------------------------------------------ b''. splitting by markers
constexpr int kErodeSide = kTile + 2 * kMaxSplit;      // 48
constexpr int kGrowSide = kTile + 2 * kMaxGrow;        // 64

// core[p] = 1.f iff the (2r+1)^2 square round p lies in `maps > threshold` (outside the image: background), else 0.f -- the float map
// that a.'s launches label with threshold 0.5.  One workgroup per 32x32 tile: the tile with a halo of r as bytes in LDS, then the
// minimum (AND) over 2r+1 columns, then over 2r+1 rows.  Every LDS index is below side * side <= 48 * 48.
__global__ __launch_bounds__(kThreads) void erode_kernel(const float* __restrict__ maps, float threshold, float* __restrict__ core, int H, int W, int r) {
  __shared__ unsigned char in[kErodeSide * kErodeSide];
  __shared__ unsigned char row[kErodeSide * kTile];
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile, side = kTile + 2 * r;
  const long base = (long)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < side * side; i += kThreads) {         // at most 9 rounds
    const int y = y0 - r + i / side, x = x0 - r + i % side;
    in[i] = y >= 0 && y < H && x >= 0 && x < W && maps[base + (long)y * W + x] > threshold;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < side * kTile; i += kThreads) {        // at most 6 rounds
    const int ly = i / kTile, lx = i % kTile;
    unsigned char a = 1;
    for (int d = 0; d <= 2 * r; ++d) a &= in[ly * side + lx + d];     // lx + d <= 31 + 2r < side
    row[i] = a;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTilePix / kThreads; ++k) {
    const int i = threadIdx.x + kThreads * k;
    const int ly = i / kTile, lx = i % kTile, y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    unsigned char a = 1;
    for (int d = 0; d <= 2 * r; ++d) a &= row[(ly + d) * kTile + lx]; // ly + d <= 31 + 2r < side
    core[base + (long)y * W + x] = a ? 1.f : 0.f;
  }
}

// g synchronous rounds of growth inside the mask, from `seeds` (the labels of the cores) to `out`; `rest` = 1.f where a mask pixel is
// still unlabelled (what a.'s launches label next), else 0.f.  One workgroup per 32x32 tile: labels and mask of the tile with a halo of g
// in LDS, then g rounds from one label buffer to the other with one barrier each.  A pixel at distance d from the edge of the loaded
// square is right after round k whenever d >= k (its value depends on the pixels within Chebyshev distance k only, and those within the
// square are all loaded); the centre has d >= g.  The smallest label among the 8 neighbours wins: the result does not depend on the
// order in which anything runs.  Plain LDS reads and writes; nothing waits for another workgroup.
__global__ __launch_bounds__(kThreads) void grow_kernel(const float* __restrict__ maps, float threshold, const int* __restrict__ seeds,
                                                        int* __restrict__ out, float* __restrict__ rest, int H, int W, int g) {
  __shared__ int buf[2][kGrowSide * kGrowSide];
  __shared__ unsigned char msk[kGrowSide * kGrowSide];
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile, side = kTile + 2 * g, cells = side * side;
  const long base = (long)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < cells; i += kThreads) {               // at most 16 rounds
    const int y = y0 - g + i / side, x = x0 - g + i % side;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    const bool m = in && maps[base + (long)y * W + x] > threshold;
    msk[i] = m;
    buf[0][i] = m ? seeds[base + (long)y * W + x] : 0;
  }
  __syncthreads();
  for (int round = 0; round < g; ++round) {                           // g <= 16, uniform: every thread reaches every barrier
    const int* src = buf[round & 1];
    int* dst = buf[(round & 1) ^ 1];
    for (int i = threadIdx.x; i < cells; i += kThreads) {
      int l = src[i];
      if (l == 0 && msk[i]) {
        const int ly = i / side, lx = i % side;
        unsigned best = ~0u;                                          // label - 1 as unsigned: 0 (no label) becomes the largest value
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int ny = ly + dy, nx = lx + dx;
            if ((dy || dx) && ny >= 0 && ny < side && nx >= 0 && nx < side) best = min(best, (unsigned)src[ny * side + nx] - 1u);
          }
        l = (int)(best + 1u);
      }
      dst[i] = l;
    }
    __syncthreads();
  }
  const int* fin = buf[g & 1];
#pragma unroll
  for (int k = 0; k < kTilePix / kThreads; ++k) {
    const int i = threadIdx.x + kThreads * k;
    const int ly = i / kTile, lx = i % kTile, y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const int c = (ly + g) * side + lx + g;
    out[base + (long)y * W + x] = fin[c];
    rest[base + (long)y * W + x] = (msk[c] && fin[c] == 0) ? 1.f : 0.f;
  }
}

// the grown regions and the labelled leftovers are disjoint: take whichever is there
__global__ __launch_bounds__(kThreads) void merge_labels_kernel(int* __restrict__ labels, const int* __restrict__ rest, long n) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p < n && labels[p] == 0) labels[p] = rest[p];
}

bool split_ok(int split_px, int grow_iters) { return split_px >= 1 && split_px <= kMaxSplit && grow_iters >= 0 && grow_iters <= kMaxGrow; }

// ------------------------------------------------------------------------------------------------ b. b'. b''. the fit pipeline on the host
// One pipeline, two instantiations: kRegions = false labels `maps > threshold` into the workspace first (dd_component_boxes, dd_component_obb),
// kRegions = true fits the caller's label image (dd_labelled_boxes, dd_labelled_obb).  `who` is the entry's name, for the messages.
struct FitWs {
  int* labels;        // components only
  Stats* stats;
  int *top;           // label image only
  int *rowcnt, *rowbase;
  Obb* recs;          // oriented only
};

// components: labels | stats | rowcnt | rowbase | recs; label image: stats | top | rowcnt | rowbase | recs.  Every part starts 16-byte aligned.
FitWs fit_ws(void* workspace, bool regions, int batch, int H, int W) {
  const long n = (long)batch * H * W, ints = align16(n * (long)sizeof(int)), rows = align16((long)batch * H * (long)sizeof(int));
  char* p = (char*)workspace;
  FitWs w{};
  if (!regions) { w.labels = (int*)p; p += ints; }
  w.stats = (Stats*)p; p += n * (long)sizeof(Stats);
  if (regions) { w.top = (int*)p; p += ints; }
  w.rowcnt = (int*)p; p += rows;
  w.rowbase = (int*)p; p += rows;
  w.recs = (Obb*)p;
  return w;
}

// refuses with the entry's limits in the message
bool fit_shape_ok(const char* who, bool oriented, int batch, int H, int W, int max_boxes) {
  if (oriented ? obb_shape_ok(batch, H, W, max_boxes) : shape_ok(batch, H, W)) return true;
  if (oriented)
    dd_fail(DD_ERR_UNSUPPORTED, "%s: batch in [1,%d], height and width in [1,%d] (the second moments are exact in 64-bit integers up to "
            "there), max_boxes in [1,%d] (got %d x %d x %d, max_boxes %d)", who, kMaxBatch, kObbMaxSide, kObbMaxBoxes, batch, H, W, max_boxes);
  else
    dd_fail(DD_ERR_UNSUPPORTED, "%s: batch in [1,%d], height and width in [1,%d] (got %d x %d x %d)", who, kMaxBatch, kMaxSide, batch, H, W);
  return false;
}

// the same for both layouts: one int and one Stats per pixel, two ints per row, one Obb per box of the oriented fit; -1 after dd_fail
int64_t fit_ws_bytes(const char* who, bool oriented, int batch, int H, int W, int max_boxes) {
  if (!fit_shape_ok(who, oriented, batch, H, W, max_boxes)) return -1;
  const long n = (long)batch * H * W;
  return align16(n * (long)sizeof(int)) + n * (long)sizeof(Stats) + 2 * align16((long)batch * H * (long)sizeof(int)) +
         (oriented ? (long)batch * max_boxes * (long)sizeof(Obb) : 0);
}

int fit_check(const char* who, bool oriented, const void* src, const float* boxes, const int32_t* counts, int min_pixels, int max_boxes, float pad_px,
              int batch, int H, int W, const void* workspace, int64_t workspace_bytes) {
  DD_REQUIRE(src && boxes && counts && workspace, DD_ERR_BAD_ARG, "%s: null pointer", who);
  DD_REQUIRE(min_pixels >= 1 && max_boxes >= 1, DD_ERR_BAD_ARG, "%s: min_pixels and max_boxes must be positive", who);
  DD_REQUIRE(!oriented || (pad_px >= 0.f && pad_px <= (float)kObbMaxSide), DD_ERR_BAD_ARG, "%s: pad_px must lie in [0,%d]", who, kObbMaxSide);
  DD_REQUIRE((uintptr_t)workspace % 16 == 0, DD_ERR_BAD_ARG, "%s: workspace must be 16-byte aligned", who);
  const int64_t need = fit_ws_bytes(who, oriented, batch, H, W, max_boxes);
  if (need < 0) return DD_ERR_UNSUPPORTED;
  DD_REQUIRE(workspace_bytes >= need, DD_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
  return 0;
}

int fit_launched(const char* who, const char* stage) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : dd_fail(DD_ERR_LAUNCH, "%s %s: %s", who, stage, hipGetErrorString(e));
}

#define FIT_LAUNCH(stage, kernel, grid, block, ...)                        \
  do {                                                                     \
    hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);            \
    if (const int rc_ = fit_launched(who, stage)) return rc_;             \
  } while (0)

// THE list of the fit's launches.  src: the maps (kRegions = false; flatten_kernel zeroes the roots' Stats) or the label image.
template <bool kRegions>
int fit_launch(const char* who, bool oriented, const void* src, float threshold, int min_pixels, int max_boxes, float pad_px, float* boxes,
               int32_t* counts, int64_t* moments, int batch, int H, int W, void* workspace, hipStream_t st) {
  const FitWs ws = fit_ws(workspace, kRegions, batch, H, W);
  const int* labels = kRegions ? (const int*)src : ws.labels;
  const dim3 runs((W + 63) / 64, (H + 3) / 4, batch), run_block(64, 4), rows(H, batch), block(kThreads);
  if constexpr (kRegions) {
    FIT_LAUNCH("init", region_init_kernel, dim3((H * W + kThreads - 1) / kThreads, batch), block, labels, ws.stats, ws.top, H * W);
  } else {
    const int rc = label_launch((const float*)src, threshold, ws.labels, ws.stats, batch, H, W, st);
    if (rc) return rc;
  }
  FIT_LAUNCH("stats", run_stats_kernel<kRegions>, runs, run_block, labels, ws.stats, H, W, ws.top);
  FIT_LAUNCH("row counts", row_count_kernel, rows, block, labels, ws.stats, ws.rowcnt, H, W, min_pixels);
  FIT_LAUNCH("row scan", row_scan_kernel, dim3(batch), block, ws.rowcnt, ws.rowbase, counts, H);
  if (!oriented) {
    FIT_LAUNCH("emit", emit_boxes_kernel<kRegions>, rows, block, labels, ws.stats, ws.rowcnt, ws.rowbase, boxes, H, W, min_pixels, max_boxes, ws.top);
    return 0;
  }
  FIT_LAUNCH("slots", obb_slot_kernel, rows, block, labels, ws.stats, ws.rowcnt, ws.rowbase, ws.recs, H, W, min_pixels, max_boxes);
  FIT_LAUNCH("moments", obb_moment_kernel<kRegions>, runs, run_block, labels, ws.stats, ws.recs, H, W, min_pixels, max_boxes);
  FIT_LAUNCH("extents", obb_extent_kernel<kRegions>, runs, run_block, labels, ws.stats, ws.recs, H, W, min_pixels, max_boxes);
  FIT_LAUNCH("emit", obb_emit_kernel, dim3((max_boxes + kThreads - 1) / kThreads, batch), block, ws.recs, counts, pad_px, boxes, (long long*)moments, H, W,
             max_boxes);
  return 0;
}

#undef FIT_LAUNCH

// ------------------------------------------------------------------------------------------------ c. IoU and ATS
__device__ __forceinline__ double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// the sine of the angle between the edges e and d is at most 1e-12: cross(e, d)^2 <= 1e-24 |e|^2 |d|^2.  Every product and sum is
// rounded on its own (no fused multiply-add, whichever way the surrounding code is contracted), so the answer does not depend on
// which of the two edges is called e: cross(d, e) is exactly -cross(e, d), and the right-hand side is a commutative product
__device__ __forceinline__ bool nearly_parallel(double ex, double ey, double dx, double dy) {
#pragma clang fp contract(off)
  const double c = ex * dy - ey * dx;
  return c * c <= 1e-24 * ((ex * ex + ey * ey) * (dx * dx + dy * dy));
}

__device__ __forceinline__ double coord(const void* p, int dtype, long i) { return dtype ? (double)((const float*)p)[i] : ((const double*)p)[i]; }

// sum of cross(p(t0), p(t1)) over the parts of P's four edges that lie inside the convex counter-clockwise quadrilateral Q.  Each
// edge is clipped to Q's four half-planes as a parameter interval [t0, t1].  An edge PARALLEL to one of Q's (to a sine of 1e-12) is
// classified from one number that both passes compute from the same operands, s = cross(dB, a - b) with A the first polygon: same
// direction -> the edge belongs to the first pass when s >= 0 and to the second when s < 0 (a shared boundary piece counts once);
// opposite direction -> interiors lie on opposite sides of a common line when s == 0, and neither pass takes it.
template <bool kFirst>
__device__ __forceinline__ double clipped_boundary(const double (&px)[4], const double (&py)[4], const double (&qx)[4], const double (&qy)[4]) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double ax = px[i], ay = py[i], dx = px[(i + 1) & 3] - ax, dy = py[(i + 1) & 3] - ay;
    double t0 = 0.0, t1 = 1.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double ex = qx[(k + 1) & 3] - qx[k], ey = qy[(k + 1) & 3] - qy[k];
      const double n0 = cross2(ex, ey, ax - qx[k], ay - qy[k]);       // > 0: the edge's start is inside half-plane k
      const double n1 = cross2(ex, ey, dx, dy);
      // parallel (nearly_parallel: the two passes see the same pair of edges with e and d exchanged, and agree on it bit for bit).
      // A copy of a box shifted along its own heading has edges on a common line whose directions differ by the rounding of the
      // corners (sine ~1e-14): -n0 / n1 is then a ratio of two rounding errors, and the shared boundary piece was counted zero,
      // one or two times by chance (IoU 1/9 came out up to 0.03 off)
      const bool par = nearly_parallel(ex, ey, dx, dy);
      if (!par && n1 > 0.0) t0 = fmax(t0, -n0 / n1);
      else if (!par && n1 < 0.0) t1 = fmin(t1, -n0 / n1);
      else {
        const double s = kFirst ? n0 : cross2(dx, dy, qx[k] - ax, qy[k] - ay);
        const bool same = ex * dx + ey * dy > 0.0;
        ok = ok && (kFirst ? (same ? s >= 0.0 : s > 0.0) : (same ? s < 0.0 : s > 0.0));
      }
    }
    if (ok && t1 > t0) acc += cross2(ax + t0 * dx, ay + t0 * dy, ax + t1 * dx, ay + t1 * dy);
  }
  return acc;
}

// ring 0,1,3,2 of box bi, translated by (-cx,-cy), made counter-clockwise; returns twice its area (>= 0)
__device__ __forceinline__ double load_ring(const void* boxes, int dtype, long bi, double cx, double cy, double (&x)[4], double (&y)[4]) {
  const long o = bi * 8;
  x[0] = coord(boxes, dtype, o + 0) - cx; y[0] = coord(boxes, dtype, o + 4) - cy;
  x[1] = coord(boxes, dtype, o + 1) - cx; y[1] = coord(boxes, dtype, o + 5) - cy;
  x[2] = coord(boxes, dtype, o + 3) - cx; y[2] = coord(boxes, dtype, o + 7) - cy;
  x[3] = coord(boxes, dtype, o + 2) - cx; y[3] = coord(boxes, dtype, o + 6) - cy;
  double a2 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) a2 += cross2(x[i], y[i], x[(i + 1) & 3], y[(i + 1) & 3]);
  if (a2 < 0.0) {
    double t = x[1]; x[1] = x[3]; x[3] = t;
    t = y[1]; y[1] = y[3]; y[3] = t;
    a2 = -a2;
  }
  return a2;
}

struct SetOffsets {       // by value in the kernel arguments, 64 samples per launch
  int first1[65], first2[65];
  long mfirst[65];        // sample s's IoU matrix [n1,n2] starts at iou[mfirst[s]]
};

__global__ __launch_bounds__(kThreads) void pair_iou_kernel(const void* __restrict__ boxes1, int dtype1, const void* __restrict__ boxes2, int dtype2,
                                                            const SetOffsets offs, float* __restrict__ iou) {
  const int s = blockIdx.y;
  const int n1 = offs.first1[s + 1] - offs.first1[s], n2 = offs.first2[s + 1] - offs.first2[s];
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (long)n1 * n2) return;
  const int i = (int)(idx / n2), j = (int)(idx % n2);
  const long bi = offs.first1[s] + i, bj = offs.first2[s] + j;
  // translate both to A's centroid: the products below are then of box-sized numbers, not of +-40 m coordinates
  double cx = 0.0, cy = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cx += coord(boxes1, dtype1, bi * 8 + k);
    cy += coord(boxes1, dtype1, bi * 8 + 4 + k);
  }
  cx *= 0.25;
  cy *= 0.25;
  double ax[4], ay[4], bx[4], by[4];
  const double area_a = 0.5 * load_ring(boxes1, dtype1, bi, cx, cy, ax, ay);
  const double area_b = 0.5 * load_ring(boxes2, dtype2, bj, cx, cy, bx, by);
  double inter = 0.5 * (clipped_boundary<true>(ax, ay, bx, by) + clipped_boundary<false>(bx, by, ax, ay));
  inter = fmin(fmax(inter, 0.0), fmin(area_a, area_b));
  const double uni = area_a + area_b - inter;
  iou[offs.mfirst[s] + idx] = uni > 0.0 ? (float)(inter / uni) : 0.f;
}

// helper.py:59-70 for one sample: iou_max over set 1 for each box of set 2, tp per threshold, ts = tp / (n1 + n2 - tp) weighted by
// 1 / threshold.  Integer counts, one fp64 evaluation by one thread: deterministic.  An empty set on either side scores 0.
__global__ __launch_bounds__(kThreads) void ats_kernel(const float* __restrict__ iou, const SetOffsets offs, float* __restrict__ ats) {
  __shared__ int tp[5];
  const int s = blockIdx.x;
  const int n1 = offs.first1[s + 1] - offs.first1[s], n2 = offs.first2[s + 1] - offs.first2[s];
  if (n1 == 0 || n2 == 0) {                                           // uniform
    if (threadIdx.x == 0) ats[s] = 0.f;
    return;
  }
  if (threadIdx.x < 5) tp[threadIdx.x] = 0;
  __syncthreads();
  const float* m = iou + offs.mfirst[s];
  const double thr[5] = {0.5, 0.6, 0.7, 0.8, 0.9};
  for (int j = threadIdx.x; j < n2; j += kThreads) {
    float best = 0.f;
    for (int i = 0; i < n1; ++i) best = fmaxf(best, m[(long)i * n2 + j]);
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if ((double)best > thr[k]) atomicAdd(&tp[k], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0, weight = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      total += (1.0 / thr[k]) * ((double)tp[k] / (double)(n1 + n2 - tp[k]));      // tp <= n2 and n1 >= 1: the denominator is positive
      weight += 1.0 / thr[k];
    }
    ats[s] = (float)(total / weight);
  }
}

int check_offsets(const int32_t* off, int batch, const char* what) {
  DD_REQUIRE(off[0] >= 0, DD_ERR_BAD_ARG, "box_iou_ats: %s offsets must be non-negative", what);
  for (int s = 0; s < batch; ++s) {
    DD_REQUIRE(off[s + 1] >= off[s], DD_ERR_BAD_ARG, "box_iou_ats: %s offsets must be non-decreasing", what);
    DD_REQUIRE(off[s + 1] - off[s] <= kMaxSet, DD_ERR_UNSUPPORTED, "box_iou_ats: at most %d boxes per sample and set (%s has %d)", kMaxSet,
               what, off[s + 1] - off[s]);
  }
  return 0;
}

}  // namespace

extern "C" {

int64_t dd_label_components_workspace_bytes(int32_t batch, int32_t height, int32_t width) {
  if (!shape_ok(batch, height, width)) {
    dd_fail(DD_ERR_UNSUPPORTED, "label_components: batch in [1,%d], height and width in [1,%d] (got %d x %d x %d)", kMaxBatch, kMaxSide, batch,
            height, width);
    return -1;
  }
  return 0;      // the labels buffer itself is the parent array
}

int dd_label_components(const float* maps, float threshold, int32_t* labels, int32_t batch, int32_t height, int32_t width, void* stream) {
  DD_REQUIRE(maps && labels, DD_ERR_BAD_ARG, "label_components: null pointer");
  DD_REQUIRE(shape_ok(batch, height, width), DD_ERR_UNSUPPORTED, "label_components: batch in [1,%d], height and width in [1,%d] (got %d x %d x %d)",
             kMaxBatch, kMaxSide, batch, height, width);
  return label_launch(maps, threshold, labels, nullptr, batch, height, width, (hipStream_t)stream);
}

int64_t dd_component_boxes_workspace_bytes(int32_t batch, int32_t height, int32_t width) {
  return fit_ws_bytes("component_boxes", false, batch, height, width, 0);
}

int dd_component_boxes(const float* maps, float threshold, int32_t min_pixels, int32_t max_boxes, float* boxes, int32_t* counts, int32_t batch,
                       int32_t height, int32_t width, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = fit_check("component_boxes", false, maps, boxes, counts, min_pixels, max_boxes, 0.f, batch, height, width, workspace, workspace_bytes);
  return rc ? rc : fit_launch<false>("component_boxes", false, maps, threshold, min_pixels, max_boxes, 0.f, boxes, counts, nullptr, batch, height, width,
                                     workspace, (hipStream_t)stream);
}

int64_t dd_component_obb_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t max_boxes) {
  return fit_ws_bytes("component_obb", true, batch, height, width, max_boxes);
}

int dd_component_obb(const float* maps, float threshold, int32_t min_pixels, int32_t max_boxes, float pad_px, float* boxes, int32_t* counts,
                     int64_t* moments, int32_t batch, int32_t height, int32_t width, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = fit_check("component_obb", true, maps, boxes, counts, min_pixels, max_boxes, pad_px, batch, height, width, workspace, workspace_bytes);
  return rc ? rc : fit_launch<false>("component_obb", true, maps, threshold, min_pixels, max_boxes, pad_px, boxes, counts, moments, batch, height, width,
                                     workspace, (hipStream_t)stream);
}

int64_t dd_split_components_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t split_px, int32_t grow_iters) {
  if (!shape_ok(batch, height, width) || !split_ok(split_px, grow_iters)) {
    dd_fail(DD_ERR_UNSUPPORTED, "split_components: batch in [1,%d], height and width in [1,%d], split_px in [1,%d], grow_iters in [0,%d] (got "
            "%d x %d x %d, split_px %d, grow_iters %d)", kMaxBatch, kMaxSide, kMaxSplit, kMaxGrow, batch, height, width, split_px, grow_iters);
    return -1;
  }
  return 2 * align16((long)batch * height * width * 4);      // one float map (cores, then leftovers) and one label image
}

int dd_split_components(const float* maps, float threshold, int32_t split_px, int32_t grow_iters, int32_t* labels, int32_t batch, int32_t height,
                        int32_t width, void* workspace, int64_t workspace_bytes, void* stream) {
  DD_REQUIRE(maps && labels && workspace, DD_ERR_BAD_ARG, "split_components: null pointer");
  DD_REQUIRE((uintptr_t)workspace % 16 == 0, DD_ERR_BAD_ARG, "split_components: workspace must be 16-byte aligned");
  const int64_t need = dd_split_components_workspace_bytes(batch, height, width, split_px, grow_iters);
  if (need < 0) return DD_ERR_UNSUPPORTED;
  DD_REQUIRE(workspace_bytes >= need, DD_ERR_WORKSPACE, "split_components: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)need);
  const long n = (long)batch * height * width;
  float* fmap = (float*)workspace;
  int* tmp = (int*)((char*)workspace + align16(n * 4));
  hipStream_t st = (hipStream_t)stream;
  const dim3 tiles((width + kTile - 1) / kTile, (height + kTile - 1) / kTile, batch);
  hipLaunchKernelGGL(erode_kernel, tiles, dim3(kThreads), 0, st, maps, threshold, fmap, height, width, split_px);
  DD_LAUNCH_CHECK("split_components erode");
  int rc = label_launch(fmap, 0.5f, tmp, nullptr, batch, height, width, st);
  if (rc) return rc;
  hipLaunchKernelGGL(grow_kernel, tiles, dim3(kThreads), 0, st, maps, threshold, (const int*)tmp, labels, fmap, height, width, grow_iters);
  DD_LAUNCH_CHECK("split_components grow");
  rc = label_launch(fmap, 0.5f, tmp, nullptr, batch, height, width, st);
  if (rc) return rc;
  hipLaunchKernelGGL(merge_labels_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, labels, (const int*)tmp, n);
  DD_LAUNCH_CHECK("split_components merge");
  return 0;
}

int64_t dd_labelled_boxes_workspace_bytes(int32_t batch, int32_t height, int32_t width) {
  return fit_ws_bytes("labelled_boxes", false, batch, height, width, 0);
}

int dd_labelled_boxes(const int32_t* labels, int32_t min_pixels, int32_t max_boxes, float* boxes, int32_t* counts, int32_t batch, int32_t height,
                      int32_t width, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = fit_check("labelled_boxes", false, labels, boxes, counts, min_pixels, max_boxes, 0.f, batch, height, width, workspace, workspace_bytes);
  return rc ? rc : fit_launch<true>("labelled_boxes", false, labels, 0.f, min_pixels, max_boxes, 0.f, boxes, counts, nullptr, batch, height, width,
                                    workspace, (hipStream_t)stream);
}

int64_t dd_labelled_obb_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t max_boxes) {
  return fit_ws_bytes("labelled_obb", true, batch, height, width, max_boxes);
}

int dd_labelled_obb(const int32_t* labels, int32_t min_pixels, int32_t max_boxes, float pad_px, float* boxes, int32_t* counts, int64_t* moments,
                    int32_t batch, int32_t height, int32_t width, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = fit_check("labelled_obb", true, labels, boxes, counts, min_pixels, max_boxes, pad_px, batch, height, width, workspace, workspace_bytes);
  return rc ? rc : fit_launch<true>("labelled_obb", true, labels, 0.f, min_pixels, max_boxes, pad_px, boxes, counts, moments, batch, height, width,
                                    workspace, (hipStream_t)stream);
}

int64_t dd_box_iou_ats_workspace_bytes(const int32_t* offsets1, const int32_t* offsets2, int32_t batch) {
  if (!offsets1 || !offsets2 || batch < 1) {
    dd_fail(DD_ERR_BAD_ARG, "box_iou_ats: bad argument");
    return -1;
  }
  if (check_offsets(offsets1, batch, "set 1") || check_offsets(offsets2, batch, "set 2")) return -1;
  long pairs = 0;
  for (int s = 0; s < batch; ++s) pairs += (long)(offsets1[s + 1] - offsets1[s]) * (offsets2[s + 1] - offsets2[s]);
  return align16(pairs * (long)sizeof(float)) + 16;      // never zero: callers allocate it unconditionally
}

int dd_box_iou_ats(const void* boxes1, int32_t dtype1, const int32_t* offsets1, const void* boxes2, int32_t dtype2, const int32_t* offsets2,
                   float* iou, float* ats, int32_t batch, void* workspace, int64_t workspace_bytes, void* stream) {
  DD_REQUIRE(offsets1 && offsets2 && ats && batch >= 1, DD_ERR_BAD_ARG, "box_iou_ats: bad argument");
  DD_REQUIRE((dtype1 == 0 || dtype1 == 1) && (dtype2 == 0 || dtype2 == 1), DD_ERR_UNSUPPORTED, "box_iou_ats: dtype must be 0 (f64) or 1 (f32)");
  int rc = check_offsets(offsets1, batch, "set 1");
  if (rc) return rc;
  rc = check_offsets(offsets2, batch, "set 2");
  if (rc) return rc;
  DD_REQUIRE(boxes1 || offsets1[batch] == offsets1[0], DD_ERR_BAD_ARG, "box_iou_ats: null boxes1");
  DD_REQUIRE(boxes2 || offsets2[batch] == offsets2[0], DD_ERR_BAD_ARG, "box_iou_ats: null boxes2");
  if (!iou) {
    const int64_t need = dd_box_iou_ats_workspace_bytes(offsets1, offsets2, batch);
    DD_REQUIRE(workspace && workspace_bytes >= need, DD_ERR_WORKSPACE, "box_iou_ats: workspace of %lld bytes, %lld needed (or pass iou)",
               (long long)workspace_bytes, (long long)need);
    iou = (float*)workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  long mbase = 0;
  for (int s0 = 0; s0 < batch; s0 += 64) {
    const int ns = min(64, batch - s0);
    SetOffsets offs;
    long most = 0;
    for (int i = 0; i <= 64; ++i) {
      const int s = s0 + min(i, ns);
      offs.first1[i] = offsets1[s];
      offs.first2[i] = offsets2[s];
      offs.mfirst[i] = mbase;
      if (i < ns) {
        const long pairs = (long)(offsets1[s + 1] - offsets1[s]) * (offsets2[s + 1] - offsets2[s]);
        most = pairs > most ? pairs : most;
        mbase += pairs;
      }
    }
    if (most > 0) {
      hipLaunchKernelGGL(pair_iou_kernel, dim3((unsigned)((most + kThreads - 1) / kThreads), ns), dim3(kThreads), 0, st, boxes1, dtype1, boxes2,
                         dtype2, offs, iou);
      DD_LAUNCH_CHECK("box_iou_ats pairs");
    }
    hipLaunchKernelGGL(ats_kernel, dim3(ns), dim3(kThreads), 0, st, (const float*)iou, offs, ats + s0);
    DD_LAUNCH_CHECK("box_iou_ats reduce");
  }
  return 0;
}

}  // extern "C"
