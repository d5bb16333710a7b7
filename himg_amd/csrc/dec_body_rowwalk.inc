  // The walk needs where the FRES payload starts and ends -- which k_dec_parse knows
  // only after its tree recovery.  It finds both by itself (the same chunk
  // look-ups, then only the LENGTH of the serialised tree: a leaf is 1 + 9 bits, a
  // branch 1 bit, pre-order, huffman_dec.cpp:152-229) and so runs beside k_dec_parse
  // instead of behind it.  Whatever is wrong with the headers or the tree is
  // k_dec_parse's to report; this kernel reports the row headers only, in
  // walk_status, which k_row_count / k_dec_status merge once both kernels are done.
  __shared__ uint32_t s_tree[(kTreeStride + 16) / 4];
  __shared__ uint32_t s_hdr[2];
  const int f = blockIdx.x, lane = threadIdx.x;
  DecFrame *df = ws.frames + f;
  const uint8_t *p = packed + (size_t)f * in_stride;
  uint32_t q = 0, end = 0;
  int r = 0;
  if (resume) {
    if (lane != 0) return;
    q = df->walk_q; r = (int)df->walk_r; end = df->walk_end;
    if (q == 0) return;   // finished (or never started): the verdict is in
  } else {
    const uint32_t n = sizes[f];
    if (lane == 0) {
      uint32_t idx = 12, sz = 0;
      bool ok = n >= 12;
      const uint32_t tags[6] = {0x544d5246u /*FRMT*/, 0x50414d4cu /*LMAP*/, 0x5345524cu /*LRES*/,
                                0x47464351u /*QCFG*/, 0x50414d46u /*FMAP*/, 0x53455246u /*FRES*/};
      for (int t = 0; ok && t < 6; ++t) {   // the order of k_dec_parse (decoder.cpp:144-290)
        ok = find_chunk(p, n, &idx, tags[t], &sz);
        if (ok && t < 5) idx += sz;
      }
      s_hdr[0] = ok ? idx : 0u;
      s_hdr[1] = ok ? sz : 0u;
      df->walk_status = 0;
      df->rows_first = 0;
      df->walk_q = 0;
    }
    __syncthreads();
    const uint32_t coff = s_hdr[0], csz = s_hdr[1];
    if (coff == 0) return;
    const uint32_t cnt = csz < (uint32_t)kTreeStride ? csz : (uint32_t)kTreeStride;
    for (uint32_t k = lane; k < (uint32_t)kTreeStride + 16u; k += 64u)
      reinterpret_cast<uint8_t *>(s_tree)[k] = k < cnt ? p[coff + k] : (uint8_t)0;
    __syncthreads();
    if (lane != 0) return;
    uint32_t bit = 0;
    {
      // Length of the serialised tree over a 64-bit register window.
      unsigned long long win = ((unsigned long long)s_tree[1] << 32) | s_tree[0];
      uint32_t next = 2, ahead = s_tree[2];
      const uint32_t bit_end = 8u * cnt;
      int open = 1, count = 0, nb = 64;
      while (open > 0) {
        if (count >= kMaxNodes || bit >= bit_end) return;   // k_dec_parse rejects this tree
        ++count;
        if (nb <= 32) { win |= (unsigned long long)ahead << nb; nb += 32; ahead = s_tree[++next]; }
        if (win & 1ull) {
          if (bit + 10u > bit_end) return;
          win >>= 10; nb -= 10; bit += 10u;
          --open;
        } else {
          win >>= 1; nb -= 1; bit += 1u;
          ++open;
        }
      }
    }
    q = coff + ((bit + 7u) >> 3);   // AlignToByte, huffman_dec.cpp:229
    end = coff + csz;
    if (q >= end) return;                    // nothing behind the tree: k_dec_parse's verdict
    df->rows_first = q;
    if (g.fix_t2 && g.rows == 1) {   // the encoder writes one block row without a size header
      ws.row_off[(size_t)f * g.rows] = q;
      ws.row_len[(size_t)f * g.rows] = end - q;
      return;
    }
  }
  uint32_t *ro = ws.row_off + (size_t)f * g.rows, *rl = ws.row_len + (size_t)f * g.rows;
  int st = 0;
  while (q != end && r < row_end) {
    if (q + 2 > end) { st = fmt_err(7, 1); break; }
    uint32_t len = p[q] | (p[q + 1] << 8);
    q += 2;
    if (len & 0x8000u) {
      if (q + 2 > end) { st = fmt_err(7, 1); break; }
      len = (len & 0x7fffu) | ((uint32_t)(p[q] | (p[q + 1] << 8)) << 15);
      q += 2;
    }
    if (len > end - q) { st = fmt_err(7, 1); break; }
    if (r < g.rows) { ro[r] = q; rl[r] = len; }
    ++r;
    q += len;
  }
  if (st || q == end) {
    if (!st && r < g.rows) st = fmt_err(7, 1);  // fewer blocks than block rows
    df->walk_status = st;
    df->walk_q = 0;
  } else {   // the next launch goes on from here
    df->walk_q = q; df->walk_r = (uint32_t)r; df->walk_end = end;
  }
