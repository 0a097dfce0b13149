// The three kernels of the rank-B optimizer pass.  adam_rankb.hip includes this text TWICE, with two definitions of
//   RANKB_KERNEL(name)   the kernel's declarator
//   RANKB_ENTER          its first statement
// once for the kernels behind dd_adam_step_rankb (the gradient scale by value in RankbArgs) and once for those behind
// dd_adam_step_rankb_dev (the scale read from device memory when the kernel starts).  Compiled twice rather than called from two
// wrappers: moved into a function that both kernels inline, the same text comes out of the compiler with other registers and another
// schedule, and the first set runs beside the conv backward on a budget of 72 registers that was measured, not estimated.
// (No include guard, no #pragma once.)

// LONG rows (many k-tiles per n-group: the encoder's fc1).  MC = 32-row chunks of the batch (1: rows <= 32; 2: rows <= 64, the gathered
// factors of two ranks); LDS 8 KB (X) + MC x 8 KB (dY): fits beside the c2 weight gradient's 133 KB.
template <int MC, int RG>
RANKB_KERNEL(lds_kernel) {
  RANKB_ENTER
  __shared__ __attribute__((aligned(16))) float xl[32 * 64];
  __shared__ __attribute__((aligned(16))) float yl[MC * 32 * 64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const __amdgpu_buffer_rsrc_t xs = dd_rsrc(a.x, a.M * a.K * 4), ys = dd_rsrc(a.dy, a.M * a.N * 4);
  const int lo = min((int)blockIdx.x * a.per, a.total), hi = min(lo + a.per, a.total);
  if (lo >= hi) return;
  int gq = lo / a.ntile_k;
  int kt = lo - gq * a.ntile_k;
  int group_in_lds = -1;
  const int nfill = (hi - lo) * MC;                       // fills of xl: (tile, chunk) pairs, chunk fastest

  // Register discipline (the budget is 72, of which 16 are accumulators, 8 the X tile in flight and 24 the p / m / v in flight):
  // nothing lane-dependent is kept across the loop that one or two instructions can rebuild, so every phase starts from a FRESH lane id
  // (dd_fresh_lane: opaque to the optimiser, which otherwise hoists a dozen addresses and masks out of the loop and keeps them).
  // Staging role of a thread: rows srow = tid / 16 and srow + 16 of a 32-row chunk, 16 bytes at column 4 (tid % 16).
  f32x4 xr0, xr1;
  auto fetch_x = [&](int tile_kt, int c) {                // X of a fill -> xr0 / xr1 (zeros past M by the descriptor, past K by the select)
    const int t = wave * 64 + dd_fresh_lane();
    const bool ok = tile_kt * 64 + 4 * (t & 15) < a.K;
    const int off = ((t >> 4) * a.K + (ok ? 4 * (t & 15) : 0)) * 4;
    const int so = (c * 32 * a.K + tile_kt * 64) * 4;
    const f32x4 v0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, off, so, 0));
    const f32x4 v1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, off, so + 16 * a.K * 4, 0));
    xr0 = ok ? v0 : f32x4{0.f, 0.f, 0.f, 0.f};
    xr1 = ok ? v1 : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  fetch_x(kt, 0);

  f32x4 acc0, acc1, acc2, acc3;
  int f = 0;
  for (int it = lo; it < hi; ++it) {
    const int nt = gq * 4 + wave;
    for (int c = 0; c < MC; ++c, ++f) {
      __syncthreads();                                    // every wave is done with the previous fill's xl (and the previous group's yl)
      {
        const int t = wave * 64 + dd_fresh_lane();
        *(f32x4*)(xl + t * 4) = xr0;                      // row t / 16, column 4 (t % 16): [row][64]
        *(f32x4*)(xl + 16 * 64 + t * 4) = xr1;
        if (gq != group_in_lds) {                         // workgroup-uniform: first tile of an n-group in this workgroup's piece
          const int col = gq * 64 + 4 * (t & 15);
          const bool ok = col < a.N;                      // N % 4 == 0 (host check)
#pragma unroll
          for (int j = 0; j < 2 * MC; ++j) {
            const int row = (t >> 4) + 16 * j;
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ys, (row * a.N + (ok ? col : 0)) * 4, 0, 0));
            // columns swizzled by the row's low bits: the four batch rows a matrix instruction reads together land in four different
            // bank groups (plain [row][64] puts all four on the same 16 banks)
            *(f32x4*)(yl + row * 64 + ((4 * (t & 15)) ^ (16 * (row & 3)))) = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
          }
          group_in_lds = gq;
        }
      }
      __syncthreads();
      if (f + 1 < nfill) {                                // the next fill's X: in flight through this fill's MFMAs and the tile's epilogue
        const bool wrap = (c + 1 == MC);
        fetch_x(wrap ? (kt + 1 == a.ntile_k ? 0 : kt + 1) : kt, wrap ? 0 : c + 1);
      }
      if (c == 0) acc0 = acc1 = acc2 = acc3 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (nt < a.ntile_n) {
        const int lane = dd_fresh_lane();
        const int r = lane & 15, q = lane >> 4;           // batch row 4 s + q of the chunk: its low bits are q
        rankb_mfma_chunk(yl + (c * 32 + q) * 64 + ((16 * wave + r) ^ (16 * q)), xl + q * 64 + 4 * r, a.M - c * 32, acc0, acc1, acc2, acc3);
      }
    }
    if (nt < a.ntile_n) {
      rankb_epilogue<RG>(a, nt, kt, acc0, acc1, acc2, acc3);
      if (a.bp && kt == 0) rankb_bias(a, yl, nt, wave);
    }
    gq += (kt + 1 == a.ntile_k);
    kt = (kt + 1 == a.ntile_k) ? 0 : kt + 1;
  }
}

// The same pass when it runs BY ITSELF (bf16 models: after the backward, dd_set_adam_blocks_per_cu > 1; no register or LDS budget): a tile
// of ONE n-tile (16 weight rows) x 256 columns, the four waves on four adjacent 64-column slabs of the same rows.  Above, a workgroup's
// tile is 64 rows x 64 columns: 256 bytes of 64 different rows (16 MB apart for the 2x-resolution fc1) per tensor and visit -- 49 k DRAM
// streams advancing 256 bytes at a time across the chip, which some boxes of the pool serve at 5.2 TB/s where a contiguous stream gets
// 5.7-6.1.  Here a visit is 1 KB of 16 rows.  X tile 32 x 256 (32 KB), one tile ahead in 32 registers; dY tile as above (its first n-tile).
RANKB_KERNEL(wide_kernel) {
  RANKB_ENTER
  __shared__ __attribute__((aligned(16))) float xl[32 * 256];
  __shared__ __attribute__((aligned(16))) float yl[32 * 64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const __amdgpu_buffer_rsrc_t xs = dd_rsrc(a.x, a.M * a.K * 4), ys = dd_rsrc(a.dy, a.M * a.N * 4);
  const int ntk = (a.K + 255) / 256;                       // 256-column tiles per n-tile; the list is (n-tile, tile), tile fastest
  const int lo = min((int)blockIdx.x * a.per, a.total), hi = min(lo + a.per, a.total);
  if (lo >= hi) return;
  int nt = lo / ntk;
  int kt = lo - nt * ntk;
  int nt_in_lds = -1;
  f32x4 xr[8];                                              // thread t: batch rows t / 16 and t / 16 + 16, columns 64 j + 4 (t % 16), j = 0 .. 3
  auto fetch_x = [&](int tile) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = tile * 256 + 64 * j + 4 * (t & 15);
      const bool ok = col < a.K;
      const int off = ((t >> 4) * a.K + (ok ? col : 0)) * 4;
      const f32x4 v0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, off, 0, 0));
      const f32x4 v1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, off, 16 * a.K * 4, 0));
      xr[2 * j] = ok ? v0 : f32x4{0.f, 0.f, 0.f, 0.f};
      xr[2 * j + 1] = ok ? v1 : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  fetch_x(kt);
  for (int it = lo; it < hi; ++it) {
    __syncthreads();                                        // every wave is done with the previous tile's xl (and the previous n-tile's yl)
    {
      const int t = threadIdx.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *(f32x4*)(xl + (t >> 4) * 256 + 64 * j + 4 * (t & 15)) = xr[2 * j];
        *(f32x4*)(xl + ((t >> 4) + 16) * 256 + 64 * j + 4 * (t & 15)) = xr[2 * j + 1];
      }
      if (nt != nt_in_lds) {                                // dY columns 16 nt .. 16 nt + 63 (the first 16 are this n-tile's), swizzled as above
        const int col = nt * 16 + 4 * (t & 15);
        const bool ok = col < a.N;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int row = (t >> 4) + 16 * j;
          const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ys, (row * a.N + (ok ? col : 0)) * 4, 0, 0));
          *(f32x4*)(yl + row * 64 + ((4 * (t & 15)) ^ (16 * (row & 3)))) = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        nt_in_lds = nt;
      }
    }
    __syncthreads();
    const bool last_of_row = kt + 1 == ntk;
    if (it + 1 < hi) fetch_x(last_of_row ? 0 : kt + 1);     // the next tile's X: in flight through this tile's MFMAs and epilogue
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
    {
      const int lane = dd_fresh_lane();
      const int r = lane & 15, q = lane >> 4;
      rankb_mfma_chunk<256>(yl + q * 64 + (r ^ (16 * q)), xl + q * 256 + 64 * wave + 4 * r, a.M, acc0, acc1, acc2, acc3);
    }
    rankb_epilogue<2>(a, nt, 4 * kt + wave, acc0, acc1, acc2, acc3);      // (returns at once for a slab past K)
    if (a.bp && kt == 0 && wave == 0) rankb_bias(a, yl, nt, 0);
    nt += last_of_row;
    kt = last_of_row ? 0 : kt + 1;
  }
}

// SHORT rows (one or two k-tiles per n-group: the road-map head K = 64, the decoder's fc2 K = 128; rows <= 32).  Here the roles swap: X
// (32 x K, at most 16 KB) is the same for every tile and stays in LDS for the whole launch, and it is the dY tile that changes -- with
// every n-group, i.e. every one or two tiles -- so dY is what travels one group ahead through the 8 prefetch registers.  A tile again
// costs the two round trips of its p / m / v only (the long-row form run on these shapes reloads dY behind a barrier for every tile:
// 0.77 ms for the head beside the c2 weight gradient against 0.2 alone).  NK = k-tiles per group (1 or 2); LDS NK x 8 KB + 8 KB.
template <int NK, int RG>
RANKB_KERNEL(short_kernel) {
  RANKB_ENTER
  __shared__ __attribute__((aligned(16))) float xl[NK * 32 * 64];
  __shared__ __attribute__((aligned(16))) float yl[32 * 64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const __amdgpu_buffer_rsrc_t xs = dd_rsrc(a.x, a.M * a.K * 4), ys = dd_rsrc(a.dy, a.M * a.N * 4);
  const int lo = min((int)blockIdx.x * a.per, a.total), hi = min(lo + a.per, a.total);      // here the list is of n-GROUPS (host: total, per)
  if (lo >= hi) return;
  {                                                       // X, once: [k-tile][row][64]
    const int t = wave * 64 + dd_fresh_lane();
#pragma unroll
    for (int k2 = 0; k2 < NK; ++k2) {
      const bool ok = k2 * 64 + 4 * (t & 15) < a.K;
      const int off = ((t >> 4) * a.K + (ok ? k2 * 64 + 4 * (t & 15) : 0)) * 4;
      const f32x4 v0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, off, 0, 0));
      const f32x4 v1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, off, 16 * a.K * 4, 0));
      *(f32x4*)(xl + k2 * 2048 + t * 4) = ok ? v0 : f32x4{0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(xl + k2 * 2048 + 1024 + t * 4) = ok ? v1 : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  f32x4 yr0, yr1;                                         // the dY tile of an n-group in flight: rows t / 16 and t / 16 + 16, 4 columns
  auto fetch_y = [&](int group) {
    const int t = wave * 64 + dd_fresh_lane();
    const int col = group * 64 + 4 * (t & 15);
    const bool ok = col < a.N;                            // N % 4 == 0 (host check); a group past the last one: all zeros, never used
    const int off = ((t >> 4) * a.N + (ok ? col : 0)) * 4;
    const f32x4 v0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ys, off, 0, 0));
    const f32x4 v1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ys, off, 16 * a.N * 4, 0));
    yr0 = ok ? v0 : f32x4{0.f, 0.f, 0.f, 0.f};
    yr1 = ok ? v1 : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  fetch_y(lo);
  for (int gq = lo; gq < hi; ++gq) {
    const int nt = gq * 4 + wave;
    __syncthreads();                                      // every wave is done with the previous group's yl (first trip: X is written)
    {
      const int t = wave * 64 + dd_fresh_lane();
      const int row = t >> 4;                             // (row + 16) & 3 == row & 3: one swizzle for both rows
      *(f32x4*)(yl + row * 64 + ((4 * (t & 15)) ^ (16 * (row & 3)))) = yr0;
      *(f32x4*)(yl + (row + 16) * 64 + ((4 * (t & 15)) ^ (16 * (row & 3)))) = yr1;
    }
    __syncthreads();
    fetch_y(gq + 1);                                      // in flight through this group's MFMAs and epilogues
    if (nt < a.ntile_n) {
#pragma nounroll
      for (int kt = 0; kt < NK; ++kt) {                   // one tile at a time: two accumulator sets alive at once would not fit the budget
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
        const int lane = dd_fresh_lane();
        const int r = lane & 15, q = lane >> 4;
        rankb_mfma_chunk(yl + q * 64 + ((16 * wave + r) ^ (16 * q)), xl + kt * 2048 + q * 64 + 4 * r, a.M, acc0, acc1, acc2, acc3);
        rankb_epilogue<RG>(a, nt, kt, acc0, acc1, acc2, acc3);
      }
      if (a.bp) rankb_bias(a, yl, nt, wave);
    }
  }
}

