// The body of k_tile_fwd and of its window source form k_tile_fwd_w: one copy, included behind each
// kernel's own parameters with FAST, COLS, QI and kWin defined (frames: a pointer to packed frames, or
// a WinSrc), so that k_tile_fwd keeps its code instruction for instruction.
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = blockIdx.y + v0, f = blockIdx.z;
  if (u >= g.cols) return;
  const uint8_t *img = frame_base(frames, g, f);
  const int bw = min(8, g.W - 8 * u), bh = min(8, g.H - 8 * v);
  const int u2 = min(u + 1, g.cols - 1), v2 = min(v + 1, g.rows - 1);
  uint8_t *dst_row = fres_sym + (size_t)f * fres_stride + (size_t)v * g.row_block + u;
  const uint8_t *row0 = img + ((long long)(8 * v) * g.W + 8 * u) * 4;   // (FAST alone reads through these two)
  const size_t pitch = (size_t)g.W * 4;

#pragma unroll 1
  for (int c = 0; c < g.C; ++c) {
    const uint8_t *m = low + (size_t)f * plane_stride + (size_t)c * g.rows * g.cols;
    // Bilinear low-res block from the four corners (downsampled.cpp:116-169).
    int left[9], right[9];
    left[0] = m[(size_t)v * g.cols + u];   left[8] = m[(size_t)v2 * g.cols + u];
    right[0] = m[(size_t)v * g.cols + u2]; right[8] = m[(size_t)v2 * g.cols + u2];
    interp9(left);
    interp9(right);

    int b[64];
    if (FAST) {
      const int mode = (g.ycbcr && c < 3) ? (c + 1) : kChanRaw;  // wave-uniform
      if (mode == kChanRaw) residual_full_tile<kChanRaw>(row0, pitch, 8 * c, left, right, b);
      else if (mode == kChanY) residual_full_tile<kChanY>(row0, pitch, 0, left, right, b);
      else if (mode == kChanCb) residual_full_tile<kChanCb>(row0, pitch, 0, left, right, b);
      else residual_full_tile<kChanCr>(row0, pitch, 0, left, right, b);
    } else {
      // Partial tiles replicate the last valid pixel of the row, rows below the
      // image repeat the bottom-right valid pixel (encoder.cpp:26-52).
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        int a[9];
        a[0] = left[y]; a[8] = right[y];
        interp9(a);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          const int yy = y < bh ? y : bh - 1;
          const int xx = y < bh ? min(x, bw - 1) : bw - 1;
          int ch[4];
          if constexpr (kWin) load_pixel(img, g, 8 * u + xx, 8 * v + yy, ch, win_pitch(frames));
          else load_pixel(img, g, 8 * u + xx, 8 * v + yy, ch);
          b[y * 8 + x] = ch[c] - a[x];
        }
      }
    }
    // Forward 2-D WHT: rows, then columns (hadamard.cpp:78-88).
#pragma unroll
    for (int y = 0; y < 8; ++y)
      wht8(b[y * 8 + 0], b[y * 8 + 1], b[y * 8 + 2], b[y * 8 + 3], b[y * 8 + 4], b[y * 8 + 5],
           b[y * 8 + 6], b[y * 8 + 7]);
#pragma unroll
    for (int x = 0; x < 8; ++x)
      wht8(b[x], b[8 + x], b[16 + x], b[24 + x], b[32 + x], b[40 + x], b[48 + x], b[56 + x]);

    const bool chroma = g.ycbcr && (c == 1 || c == 2);  // encoder.cpp:284
    const uint8_t *shift = nullptr;
    KargWords shift_w = nullptr;
    if constexpr (QI) shift_w = uniform_words(qual_entry(st, f)->st.s[chroma ? 1 : 0]);
    else shift = st.s[chroma ? 1 : 0];
    const int cols = COLS ? COLS : g.cols;  // compile-time stride -> no 64 live store addresses
    uint8_t *dst = dst_row + (size_t)c * 64 * cols;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const int pos = kScan[i];
      int s;
      if constexpr (QI) s = (int)((shift_w[pos >> 2] >> (8 * (pos & 3))) & 255u);
      else s = shift[pos];
      const int x = (int)(int16_t)b[pos];  // the reference's int16 wrap
      // Sign-magnitude rounding shift (quantize.cpp:135-148).
      const int r = s ? (1 << (s - 1)) : 0;
      const int mag = x < 0 ? ((-x + r) >> s) : ((x + r) >> s);
      // Companding (mapper.cpp:159-182): the full-res table is the identity up to
      // 50; larger magnitudes go through the LUT of the restated search.
      uint32_t code = (uint32_t)mag;
      if (mag > 50) code = fmap_lut[mag];
      dst[(size_t)i * cols] = (x < 0) ? (uint8_t)(0u - code) : (uint8_t)code;
    }
  }
