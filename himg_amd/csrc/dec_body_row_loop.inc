// The persistent row loop of k_dec_row_fused and of its tensor, pitched, pyramid and planes forms
// (k_dec_row_fused_t / _p / _m / _c): one copy, included as each kernel's whole body with KA (the kernel's
// argument struct), kRowTens / kRowPitch / kRowPyr / kRowPlanes (the form) and HIMG_ROW_A (the RowArgs inside KA)
// defined, so that every kernel keeps its code instruction for instruction.  A function template
// around the loop does not: DESIGN.md 4.12.
  typedef const __attribute__((address_space(4))) KA *KArgs;
  KArgs ka = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t total = (uint32_t)HIMG_ROW_A(ka).gx * (uint32_t)HIMG_ROW_A(ka).gy, S = gridDim.x;
  // Round i: the grid elements [i S, (i + 1) S), this workgroup the one at (blockIdx.x + 37 i) mod S
  // -- rotated, or a workgroup would meet the same row positions of every frame (S = 256, 512 rows
  // per frame: two of them) and the slow rows of similar frames would all be one workgroup's:
  // 128 identical frames 10.28 ms against 10.01 with a workgroup per row.
  auto element = [&](uint32_t i) { return i * S + (blockIdx.x + 37u * i) % S; };
  bool again = false;
  int f_prev = -1;
#pragma unroll 1
  for (uint32_t i = 0; i * S < total; ++i) {
    const uint32_t lin = element(i);
    if (lin >= total) break;   // (the last round is a partial one)
    asm volatile("" : "+s"(ka));
    Geom g;
    DecWs ws;
    karg_copy<uint32_t>(&g, &HIMG_ROW_A(ka).g);
    karg_copy<unsigned long long>(&ws, &HIMG_ROW_A(ka).ws);
    const int gx = HIMG_ROW_A(ka).gx, f = (int)(lin / (uint32_t)gx);
    const uint32_t nd = (uint32_t)HIMG_ROW_A(ka).next_dist;
    dec_row_fused_body<COLS, kRowTens, kRowPitch, kRowPyr, kRowPlanes>(
        g, ws, HIMG_ROW_A(ka).packed, HIMG_ROW_A(ka).in_stride, HIMG_ROW_A(ka).sizes, HIMG_ROW_A(ka).out_frames,
        HIMG_ROW_A(ka).r0, HIMG_ROW_A(ka).r1, HIMG_ROW_A(ka).rpw, (int)(lin % (uint32_t)gx), f, gx, HIMG_ROW_A(ka).gy,
        nd ? lin + nd : element(i + 1), again, f == f_prev, row_td(ka), row_pd(ka), row_pm(ka), row_pc(ka));
    again = true;
    f_prev = f;
  }
