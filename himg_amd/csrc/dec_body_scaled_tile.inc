// The body of scaled_tile_rows and scaled_tile_rows_crop (kernels_dec.hip) in front of their stores: one
// tile's samples at scale S / 8, output rows Y0 .. Y0 + NY - 1, finished (colour inverse included) in
// q[(Y - Y0) * S + X], the pixel's channels in bytes 0..3.  Included, not called: k_dec_scaled keeps its
// code instruction for instruction, and there is one copy of the arithmetic.
  constexpr int F = 8 / S, LG = S == 4 ? 1 : 2;
  const int cols = g.cols, C = g.C;
  const int v2 = min(v + 1, g.rows - 1), u2 = min(u + 1, cols - 1);
  uint32_t q[NY * S];   // [(Y - Y0) * S + X]: the pixel's channels in bytes 0..3
#pragma unroll
  for (int i = 0; i < NY * S; ++i) q[i] = 0u;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {   // (not unrolled: four planes' loads in flight at once cost registers)
    const uint8_t *m = low + (size_t)c * g.rows * cols;
    const int chroma = (ycbcr && (c == 1 || c == 2)) ? 1 : 0;  // decoder.cpp:376
    const uint8_t *sh = s_shift + chroma * 64;
    // quantize.cpp:153-165 on the top-left S x S: d[j][i], row j, column i.
    int d[S][S];
#pragma unroll
    for (int k = 0; k < S * S; ++k) {
      const int pos = kScanD[k], j = pos >> 3, i = pos & 7;
      const uint32_t code = sym[(size_t)c * cstride + (size_t)k * sstride];
      d[j][i] = (int)(int16_t)(uint16_t)((uint32_t)(int)s_unmap[code] << sh[pos]);
    }
#pragma unroll
    for (int j = 0; j < S; ++j) iwht_short<S>(d[j]);   // rows: d[j][X]
    int p[S][S];
#pragma unroll
    for (int X = 0; X < S; ++X) {
      int col[S];
#pragma unroll
      for (int j = 0; j < S; ++j) col[j] = d[j][X];
      iwht_short<S>(col);
#pragma unroll
      for (int Y = 0; Y < S; ++Y) p[Y][X] = col[Y];
    }
    // The low-res block (downsampled.cpp:130-169) and its F x F box means, an output row at a time.
    // The left and the right column are interpolated together, one in each half of a register
    // (values below 256: the bit a half's sum hands down is masked away).
    uint32_t lr[9];
    lr[0] = (uint32_t)m[(size_t)v * cols + u] | ((uint32_t)m[(size_t)v * cols + u2] << 16);
    lr[8] = (uint32_t)m[(size_t)v2 * cols + u] | ((uint32_t)m[(size_t)v2 * cols + u2] << 16);
    interp9pk(lr);
#pragma unroll
    for (int Y = Y0; Y < Y0 + NY; ++Y) {
      int acc[S];
#pragma unroll
      for (int X = 0; X < S; ++X) acc[X] = F * F / 2;
#pragma unroll
      for (int y = Y * F; y < Y * F + F; ++y) {
        int a[9];
        a[0] = (int)(lr[y] & 0xffffu);
        a[8] = (int)(lr[y] >> 16);
        interp9d(a);
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[x / F] += a[x];
      }
#pragma unroll
      for (int X = 0; X < S; ++X) {
        const int smp = clamp255d((int)(int16_t)(p[Y][X] + (acc[X] >> (2 * LG))));   // decoder.cpp:36-75
        q[(Y - Y0) * S + X] |= (uint32_t)smp << (8 * c);
      }
    }
  }
  if (ycbcr) {
#pragma unroll
    for (int i = 0; i < NY * S; ++i) {
      uint32_t c0 = q[i] & 255u, c1 = (q[i] >> 8) & 255u, c2 = (q[i] >> 16) & 255u;
      ycc_to_rgb(c0, c1, c2);   // ycbcr.cpp:54-82
      q[i] = (q[i] & 0xff000000u) | c0 | (c1 << 8) | (c2 << 16);
    }
  }
