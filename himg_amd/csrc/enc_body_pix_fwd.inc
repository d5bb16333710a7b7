// The body of k_pix_fwd and of its window source form k_pix_fwd_w: one copy, included behind each
// kernel's own parameters with YCBCR, COLS, FULL, QI and kWin defined (frames: a pointer to packed
// frames, or a WinSrc), so that k_pix_fwd keeps its code instruction for instruction.
  // Companding LUT for magnitudes below kPixLut (every larger one maps to 127:
  // the full-res table tops out at 8039, mapper.cpp:54-71,159-182).
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[kPixLut];
  for (int k = threadIdx.x; k < kPixLut / 16; k += kPixThreads)
    reinterpret_cast<uint4 *>(s_lut)[k] = reinterpret_cast<const uint4 *>(fmap_lut)[k];
  __syncthreads();
  const int cols = COLS ? COLS : g.cols;
  const int u = blockIdx.x * kPixThreads + threadIdx.x;
  const int v = blockIdx.y + v0, f = blockIdx.z;
  if ((int)(blockIdx.x * kPixThreads + (threadIdx.x & ~63)) >= cols) return;   // the whole wave is beyond the row
  KargWords qw = nullptr;   // QI: [rr, kk, ss][luma / chroma][coefficient], as k_front indexes PixQuant
  if constexpr (QI) qw = uniform_words(qual_entry(pq, f)->pq);
  // FULL: cols is a multiple of 64, every lane of a live wave owns a tile.
  const bool valid = FULL || u < cols;
  const int uc = valid ? u : cols - 1;
  const uint8_t *img = frame_base(frames, g, f);
  const int u2 = min(uc + 1, cols - 1), v2 = min(v + 1, g.rows - 1);
  // Wave-uniform base + 32-bit lane offset: the stores take the scalar-base form and
  // the per-coefficient stride is scalar arithmetic, not 64-bit adds per lane.
  // The symbol stores go through a buffer descriptor of the frame's symbol plane:
  // buffer_store_byte takes the lane offset in a VGPR and the (wave-uniform) offset of
  // the coefficient row in an SGPR -- no address arithmetic on the vector unit.
  const __amdgpu_buffer_rsrc_t sym_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      fres_sym + (size_t)f * fres_stride, 0, (int)g.fres_size, 0x00020000);
  const uint32_t row_off = (uint32_t)v * (uint32_t)g.row_block;
  const uint32_t lane_off = (uint32_t)uc;
  const uint8_t *row0 = kWin ? img + (size_t)(8 * v) * win_pitch(frames) + (size_t)(8 * uc) * 4
                             : img + ((long long)(8 * v) * g.W + 8 * uc) * 4;
  const size_t pitch = kWin ? win_pitch(frames) : (size_t)g.W * 4;

  // The tile: 8 rows x 8 pixels, one pass over HBM.
  uint32_t px[64];
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const SrcQuad<kWin> *rp = reinterpret_cast<const SrcQuad<kWin> *>(row0 + (size_t)y * pitch);
    const SrcQuad<kWin> q0 = rp[0], q1 = rp[1];
    px[y * 8 + 0] = q0.x; px[y * 8 + 1] = q0.y; px[y * 8 + 2] = q0.z; px[y * 8 + 3] = q0.w;
    px[y * 8 + 4] = q1.x; px[y * 8 + 5] = q1.y; px[y * 8 + 6] = q1.z; px[y * 8 + 7] = q1.w;
  }
  // Low-res corners of the four channels: (left, right) of block rows v and v + 1.
  uint32_t lr0[4], lr8[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint8_t *m = low + (size_t)f * plane_stride + (size_t)c * g.rows * cols;
    lr0[c] = (uint32_t)m[(size_t)v * cols + uc] | ((uint32_t)m[(size_t)v * cols + u2] << 8);
    lr8[c] = (uint32_t)m[(size_t)v2 * cols + uc] | ((uint32_t)m[(size_t)v2 * cols + u2] << 8);
  }

#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    // Channels in the low / high half of this pair, and their shift table.
    const int cA = YCBCR ? (pr == 0 ? 2 : 0) : (pr == 0 ? 0 : 1);
    const int cB = YCBCR ? (pr == 0 ? 1 : 3) : (pr == 0 ? 2 : 3);
    pk16 b[64];
    {
      uint32_t LA[2][8], LB[2][8];
      lowres_quads_e(lr0[cA], lr8[cA], LA);
      lowres_quads_e(lr0[cB], lr8[cB], LB);
#pragma unroll
      for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          // (low A, low B) of this pixel, zero-extended to the two halves.
          const uint32_t sel = 0x0c000c00u | (uint32_t)(y & 3) | ((uint32_t)(4 + (y & 3)) << 16);
          const pk16 lo = __builtin_bit_cast(pk16, __builtin_amdgcn_perm(LB[y >> 2][x], LA[y >> 2][x], sel));
          const pk16 pv = pr == 0 ? pix_pair<YCBCR, 0>(px[y * 8 + x]) : pix_pair<YCBCR, 1>(px[y * 8 + x]);
          b[y * 8 + x] = pv - lo;
        }
    }
    // Forward 2-D WHT: rows, then columns (hadamard.cpp:78-88).
#pragma unroll
    for (int y = 0; y < 8; ++y)
      wht8_pk(b[y * 8 + 0], b[y * 8 + 1], b[y * 8 + 2], b[y * 8 + 3], b[y * 8 + 4], b[y * 8 + 5],
              b[y * 8 + 6], b[y * 8 + 7]);
#pragma unroll
    for (int x = 0; x < 8; ++x)
      wht8_pk(b[x], b[8 + x], b[16 + x], b[24 + x], b[32 + x], b[40 + x], b[48 + x], b[56 + x]);

    const uint32_t offA = row_off + (uint32_t)(cA * 64 * cols), offB = row_off + (uint32_t)(cB * 64 * cols);
    // Quantise (quantize.cpp:127-151), compand (mapper.cpp:159-182) and store, in
    // groups of coefficients in scan order.  sign * ((|x| + r) >> s) is branch free:
    // (x + r + sign * k) >> s with sign = x >> 15 and k = [s > 0]; r, k and s come
    // as packed pairs from the kernel arguments (pq, scan order).  Companding is the
    // identity while |q| <= 50; the group keeps the largest q + 50 (as unsigned: <=
    // 100 exactly then) and ONE wave-uniform branch per group sends the group
    // through the LUT -- the first sixteen coefficients (DC and first order, the
    // ones high-contrast tiles push beyond 50) in groups of four, the rest in
    // sixteens.  (A test per coefficient was 128 compare + branch pairs per tile,
    // each behind hazard no-ops, and 128 basic blocks the scheduler could not
    // interleave across.)
    const int qt = (YCBCR && pr == 0) ? 1 : 0;
    auto group = [&](auto i0c, auto nc) {
      constexpr int I0 = decltype(i0c)::value, N = decltype(nc)::value;
      pk16 q[N];
      upk16 top = {0, 0};
      for_seq<N>([&](auto kc) {
        constexpr int k = decltype(kc)::value, i = I0 + k, pos = kScan[i];
        const pk16 x = b[pos];
        const pk16 fifteen = {15, 15};
        const pk16 sign = x >> fifteen;                       // 0 or -1 per half
        pk16 rr, kk, ss;
        if constexpr (QI) {
          rr = __builtin_bit_cast(pk16, qw[(0 * 2 + qt) * 64 + i]); kk = __builtin_bit_cast(pk16, qw[(1 * 2 + qt) * 64 + i]);
          ss = __builtin_bit_cast(pk16, qw[(2 * 2 + qt) * 64 + i]);
        } else {
          rr = __builtin_bit_cast(pk16, pq.rr[qt][i]); kk = __builtin_bit_cast(pk16, pq.kk[qt][i]);
          ss = __builtin_bit_cast(pk16, pq.ss[qt][i]);
        }
        q[k] = (sign * kk + x + rr) >> ss;
        const upk16 fifty = {50, 50};
        top = __builtin_elementwise_max(top, (upk16)(__builtin_bit_cast(upk16, q[k]) + fifty));
      });
      const upk16 hundred = {100, 100};
      const uint32_t over = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(top, hundred));
      if (__builtin_expect(__any(over != 0u), 0)) {
        for_seq<N>([&](auto kc) {
          constexpr int k = decltype(kc)::value;
          const pk16 fifteen = {15, 15};
          const pk16 sign = q[k] >> fifteen;
          const pk16 mag = (q[k] ^ sign) - sign;
          const uint32_t ma = min((uint32_t)(uint16_t)mag.x, (uint32_t)(kPixLut - 1));
          const uint32_t mb = min((uint32_t)(uint16_t)mag.y, (uint32_t)(kPixLut - 1));
          pk16 code;                                          // the LUT is the identity below 51
          code.x = (short)s_lut[ma];
          code.y = (short)s_lut[mb];
          q[k] = (code ^ sign) - sign;
        });
      }
      if (valid) {
        for_seq<N>([&](auto kc) {
          constexpr int k = decltype(kc)::value, i = I0 + k;
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)q[k].x, sym_rsrc, lane_off, offA + (uint32_t)(i * cols), 0);
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)q[k].y, sym_rsrc, lane_off, offB + (uint32_t)(i * cols), 0);
        });
      }
    };
    using std::integral_constant;
    group(integral_constant<int, 0>{}, integral_constant<int, 4>{});
    group(integral_constant<int, 4>{}, integral_constant<int, 4>{});
    group(integral_constant<int, 8>{}, integral_constant<int, 4>{});
    group(integral_constant<int, 12>{}, integral_constant<int, 4>{});
    group(integral_constant<int, 16>{}, integral_constant<int, 16>{});
    group(integral_constant<int, 32>{}, integral_constant<int, 16>{});
    group(integral_constant<int, 48>{}, integral_constant<int, 16>{});
  }
