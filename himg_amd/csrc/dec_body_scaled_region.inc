// The body of k_dec_scaled_region<S> and of k_dec_opened_scaled_region<S>: one copy, included behind each
// kernel's own parameters (g, ws, packed, in_stride, sizes, sa) with kScaledMap, smap and wstat defined, so that
// k_dec_scaled_region keeps its code instruction for instruction.  kScaledMap (the opened-streams form; false
// and unused in k_dec_scaled_region): blockIdx.z is a WINDOW -- its origin, its output slot and its verdict word
// wstat[f] -- of stream fs = smap[f], whose frame, records, tables and planes it reads and never writes.
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int LG = S == 4 ? 1 : 2;
  const RegionLayout L = scaled_layout<S>(g.C, sa.sw);
  LdsTables &T = *reinterpret_cast<LdsTables *>(smem + L.tab);
  RegionShared *sh = reinterpret_cast<RegionShared *>(smem + L.sh);
  const int16_t *s_unmap = reinterpret_cast<const int16_t *>(smem + L.rowtab);   // unmap, shift: contiguous
  const uint8_t *s_shift = smem + L.rowtab + 512;
  uint8_t *sym = smem + L.sym;
  const int tid = threadIdx.x, f = blockIdx.z;
  int fs = f;
  if constexpr (kScaledMap) fs = __builtin_amdgcn_readfirstlane(smap[f]);
  // The frame's own window: its rows and tile columns; a workgroup past either has nothing to do.
  ScaledCrop rr;
  rr.x = sa.org[2 * f] >> LG; rr.y = sa.org[2 * f + 1] >> LG; rr.w = sa.w; rr.h = sa.h;
  const int r = rr.y / S + (int)blockIdx.y, u1 = (rr.x + rr.w + S - 1) / S;
  const int su0 = rr.x / S + (int)blockIdx.x * sa.sw;
  if (r >= (rr.y + rr.h + S - 1) / S || su0 >= u1) return;
  const int ww = min(sa.sw, u1 - su0);
  DecFrame *df = ws.frames + fs;
  if (tid == 0) {
    sh->flag = df->status; sh->err = 0; sh->endbit = ~0ull;
    if constexpr (kScaledMap) sh->flag |= wstat[f];   // (the stream's head verdict, or this window's own)
  }
  __syncthreads();
  if (sh->flag) return;
  load_dec_tables(ws, df, fs, 1, &T);
  if (tid < kRowTabWords / 4)
    reinterpret_cast<uint4 *>(smem + L.rowtab)[tid] = reinterpret_cast<const uint4 *>(df->row_tabs)[tid];
  const uint32_t nsym16 = (L.seg * (uint32_t)(S * S) * (uint32_t)g.C + 15u) / 16u;
  for (uint32_t k = tid; k < nsym16; k += kDecThreads) reinterpret_cast<uint4 *>(sym)[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  // A tree with a leaf past the last run symbol: a walk may fail anywhere (every lane walks).
  const int nn = min(df->s[1].num_nodes, kMaxNodes + 1);
  const uint32_t nd = tid < nn ? T.nd[tid] : 0u;
  const bool strict = __syncthreads_or((nn <= 1) || ((nd >> 20) != 0 && (nd >> 20) - 1u > 260u)) != 0;

  const size_t ri = (size_t)fs * g.rows + (size_t)r;
  const uint32_t pay_off = ws.row_off[ri], pay_len = ws.row_len[ri], out_size = (uint32_t)g.row_block;
  const uint8_t *p = packed + (size_t)fs * in_stride;
  const uint32_t end = (uint32_t)min((unsigned long long)sizes[fs], (unsigned long long)pay_off + pay_len);
  const GrpTables tb = tables_of(&T);
  ScaledWin<S> win;
  win.base = lds_addr(sym); win.cols = (uint32_t)g.cols; win.u0 = (uint32_t)su0; win.ww = (uint32_t)ww;
  win.seg = L.seg; win.nseg = 64u * (uint32_t)g.C;
  const uint32_t *ps = ws.lane_start + ri * kDecThreads, *po = ws.lane_off + ri * (kDecThreads + kRecHdr);
  const uint32_t valid = po[kDecThreads + 2];
  const bool rec = valid != 0 && pay_len != 0;
  const unsigned long long P1 = 8ull * pay_len;
  uint32_t end_bp = ~0u, tot = 0, rel0 = 0;
  bool ok = true;
  if (pay_len != 0) {
    GReader rd;
    rel0 = rd.attach(p, end, 8ull * pay_off);
    const uint32_t rel_end = rel0 + (uint32_t)P1;
    if (rec) {
      const uint32_t st = ps[tid], off = po[tid], nxt = po[tid + 1];
      const uint32_t nst = tid + 1 < kDecThreads ? ps[tid + 1] : ~0u;
      tot = po[kDecThreads];
      const uint32_t start = rel0 + st, wlim = nst < (uint32_t)P1 ? rel0 + nst : rel_end;
      const uint32_t cnt = nxt - off;
      if (off + cnt < out_size) {
        // The lane's last needed symbol of the window (stop), if its symbols [off, off + cnt) hold one.
        uint32_t stop = ~0u;
        bool walk = true;
        if (!strict) {
          const long long last = cnt ? scaled_last_needed<S>(off + cnt - 1u, (uint32_t)g.cols, (uint32_t)su0, (uint32_t)ww) : -1;
          walk = cnt != 0 && last >= (long long)off;
          stop = walk ? (uint32_t)last : 0u;
        }
        if (walk) ok = region_walk<false>(rd, tb, start, wlim, off, stop, out_size, win, &end_bp);
      } else if (off < out_size) {
        ok = region_walk<true>(rd, tb, start, wlim, off, ~0u, out_size, win, &end_bp);
      }
    } else if (tid == 0) {
      ok = region_walk<true>(rd, tb, rel0, rel_end, 0u, ~0u, out_size, win, &end_bp);
    }
  }
  if (!ok) sh->err = 1;
  if (end_bp != ~0u) sh->endbit = (unsigned long long)(end_bp - rel0);
  __syncthreads();
  // ---- accept / reject like UncompressStream (huffman_dec.cpp:361-417), decode_row_recorded ----
  int bad = sh->err || pay_len == 0;
  if (rec && tot < out_size) bad = 1;   // ran out of payload before the block was full
  const unsigned long long E = sh->endbit;
  if (!bad && !(E <= P1 && E + 8 > P1 && E > 0)) bad = 1;   // AtTheEnd (huffman_dec.cpp:140-145)
  if (bad) {
    if constexpr (kScaledMap) { if (tid == 0) atomicMax(&wstat[f], fmt_err(7, 1)); }
    else if (tid == 0) atomicMax(&df->status, fmt_err(7, 1));
    return;
  }
  // ---- the strip's tiles: a lane per tile, the stores cropped to the window ----
  const uint8_t *low = ws.low + (size_t)fs * ws.plane_stride;
  uint8_t *img = sa.out + (size_t)f * ((size_t)sa.h * sa.w * g.C);
  const int ycbcr = df->ycbcr;
#pragma unroll 1
  for (int ul = tid; ul < ww; ul += kDecThreads)
    scaled_tile_store_crop<S>(g, (int)L.seg, S * S * (int)L.seg, sym + 4 + ul, low, s_unmap, s_shift, ycbcr, su0 + ul,
                              r, rr, img);
