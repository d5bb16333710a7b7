  DecFrame *df = ws.frames;   // (one frame)
  const uint32_t n = sizes[0];
  int bad = 0;
  for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) {
    const uint32_t off = index[r], len = index[g.rows + r];
    ws.row_off[r] = off;
    ws.row_len[r] = len;
    if (off > n || len > n - off) bad = 1;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) { df->walk_status = bad ? fmt_err(7, 1) : 0; df->rows_first = 0; }
