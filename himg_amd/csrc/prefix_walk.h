// prefix_walk.h -- the walk over a stream PREFIX: the first `avail` bytes of a stream whose RIFF
// header declares T bytes (include/himg_hip.h, "decode a stream prefix").  One copy of the rules for
// the host (himg_hip_prefix_peek) and the device (k_span_gate, k_span_rowwalk): every load is
// checked against `avail` first, every container bound against T.
#ifndef HIMG_PREFIX_WALK_H_
#define HIMG_PREFIX_WALK_H_

#include <stdint.h>

#include "himg_dev.h"

namespace himg_dev {

// How a step of the walk ended.
//   kPfxOk      it passed, from bytes below avail alone;
//   kPfxShort   it needs a byte at or beyond avail: no verdict (HIMG_ERR_CAPACITY);
//   kPfxFormat  a check of the decoder fails on bytes below avail (HIMG_ERR_FORMAT).
enum { kPfxOk = 0, kPfxShort = 1, kPfxFormat = 2 };

struct PfxHead {
  uint32_t T;              // the size the RIFF header declares (0: not reached)
  uint32_t W, H, C, ycc;   // FRMT's fields
  int frmt;                // 1 once FRMT's fields have been read (they are untrusted: C may be 0)
  uint32_t coff, csz;      // the FRES chunk's payload: where the serialised tree starts, the chunk's size
  uint32_t need;           // the bytes the container parse stages of the chunks found so far end here
  int stage, huff;         // kPfxFormat: the decoder's stage that fails, 1 RIFF .. 7 FRES; 1: its Huffman layer's check
};

__host__ __device__ inline uint32_t pfx_rd32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// decoder.cpp:428-461 (find_chunk of kernels_dec.hip) with the bytes present checked first.
__host__ __device__ inline int pfx_find(const uint8_t *p, uint32_t avail, uint32_t T, uint32_t *idx, uint32_t tag,
                                        uint32_t *size) {
  for (;;) {
    if ((unsigned long long)*idx + 8 > T) return kPfxFormat;
    if ((unsigned long long)*idx + 8 > avail) return kPfxShort;
    const uint32_t t = pfx_rd32(p + *idx), sz = pfx_rd32(p + *idx + 4);
    *idx += 8;
    if (sz > 0x7fffffffu || (unsigned long long)*idx + sz > T) return kPfxFormat;
    if (t == tag) { *size = sz; return kPfxOk; }
    *idx += sz;
  }
}

// The chunk headers RIFF .. FRES in k_dec_parse's order, with its checks (decoder.cpp:144-290).
// row_block: the FRES symbols of a block row when the caller knows the geometry (the device), 0: taken
// from FRMT.  A kPfxFormat is final only where h->need <= avail: the parse reports the FIRST failure in
// the reference's order, and an earlier chunk's body (which it stages up to h->need) may hold one.
__host__ __device__ inline int pfx_chain(const uint8_t *p, uint32_t avail, int fix_t2, uint32_t row_block, PfxHead *h) {
  h->T = 0; h->W = h->H = h->C = h->ycc = 0; h->frmt = 0; h->coff = h->csz = 0; h->need = 0; h->stage = 1; h->huff = 0;
  if (avail < 12) return kPfxShort;
  const unsigned long long T64 = (unsigned long long)pfx_rd32(p + 4) + 8u;
  if (pfx_rd32(p) != 0x46464952u /*RIFF*/ || T64 > 0x7fffffffu || T64 < 12 || pfx_rd32(p + 8) != 0x474d4948u /*HIMG*/)
    return kPfxFormat;
  const uint32_t T = (uint32_t)T64;
  h->T = T;
  if (avail > T) return kPfxFormat;
  const uint32_t stage_max = (uint32_t)kTreeStride;
  uint32_t idx = 12, sz = 0;
  int rc;
  h->stage = 2;
  if ((rc = pfx_find(p, avail, T, &idx, 0x544d5246u /*FRMT*/, &sz)) != kPfxOk) return rc;
  if (sz < 11) return kPfxFormat;
  if ((unsigned long long)idx + 11 > avail) return kPfxShort;
  if (p[idx] != 1) return kPfxFormat;
  h->W = pfx_rd32(p + idx + 1); h->H = pfx_rd32(p + idx + 5); h->C = p[idx + 9];
  h->ycc = (p[idx + 10] != 0 && h->C >= 3) ? 1u : 0u;
  h->frmt = 1;
  idx += sz;
  const uint32_t tags[5] = {0x50414d4cu /*LMAP*/, 0x5345524cu /*LRES*/, 0x47464351u /*QCFG*/,
                            0x50414d46u /*FMAP*/, 0x53455246u /*FRES*/};
  for (int t = 0; t < 5; ++t) {
    h->stage = 3 + t;
    if ((rc = pfx_find(p, avail, T, &idx, tags[t], &sz)) != kPfxOk) return rc;
    if (t == 2 && sz != (h->ycc ? 64u : 32u)) return kPfxFormat;
    if (t == 4) break;
    const uint32_t e = idx + (sz < stage_max ? sz : stage_max);
    h->need = e > h->need ? e : h->need;
    idx += sz;
  }
  // Trap T2 (huffman_dec.cpp:215-219), as k_dec_parse judges it.
  if (!row_block) row_block = ((h->W + 7u) / 8u) * h->C * 64u;
  if (!fix_t2 && !(row_block < sz)) return h->huff = 1, kPfxFormat;
  h->coff = idx; h->csz = sz;
  return kPfxOk;
}

// The length of the serialised FRES tree (huffman_dec.cpp:152-229; dec_body_rowwalk.inc): `tree` holds
// the first `have` bytes of the chunk's payload, the chunk is csz bytes.  *bytes: the tree's length,
// AlignToByte included.  kPfxShort where the walk needs a byte of the chunk that is not among them.
__host__ __device__ inline int pfx_tree_len(const uint8_t *tree, uint32_t have, uint32_t csz, uint32_t *bytes) {
  const uint32_t cnt = csz < (uint32_t)kTreeStride ? csz : (uint32_t)kTreeStride;
  const uint32_t bit_end = 8u * cnt;
  uint32_t bit = 0;
  int open = 1, count = 0;
  while (open > 0) {
    if (count >= 2 * kNumSym - 1 || bit >= bit_end) return kPfxFormat;
    if ((bit >> 3) >= have) return kPfxShort;
    ++count;
    if ((tree[bit >> 3] >> (bit & 7u)) & 1u) {
      if (bit + 10u > bit_end) return kPfxFormat;
      bit += 10u;
      --open;
    } else {
      bit += 1u;
      ++open;
    }
  }
  *bytes = (bit + 7u) >> 3;
  return *bytes > have ? kPfxShort : kPfxOk;
}

// One row header at `q` by k_dec_rowwalk's rules (huffman_dec.cpp:232-248): two bytes of length, or four
// with the top bit of the first pair set, header and payload inside the chunk (`end`) and below `avail`.
// kPfxOk: the payload is bytes [*body, *body + *len).  kPfxShort: *need is the least avail at which the
// step passes.  (A caller that holds the whole chunk passes avail = end and sees no kPfxShort.)
__host__ __device__ inline int pfx_row_header(const uint8_t *p, uint32_t q, uint32_t end, uint32_t avail, uint32_t *body,
                                              uint32_t *len, uint32_t *need) {
  if (q + 2 > end) return kPfxFormat;
  if (q + 2 > avail) return *need = q + 2, kPfxShort;
  uint32_t n = (uint32_t)p[q] | ((uint32_t)p[q + 1] << 8), b = q + 2;
  if (n & 0x8000u) {
    if (b + 2 > end) return kPfxFormat;
    if (b + 2 > avail) return *need = b + 2, kPfxShort;
    n = (n & 0x7fffu) | (((uint32_t)p[b] | ((uint32_t)p[b + 1] << 8)) << 15);
    b += 2;
  }
  if (n > end - b) return kPfxFormat;
  if (b + n > avail) return *need = b + n, kPfxShort;
  *body = b; *len = n;
  return kPfxOk;
}

// What a walk over the row headers finds: the rows whose header and payload lie wholly below avail.
struct PfxRows {
  int k;             // complete rows, at most `rows`
  uint32_t used;     // where row k - 1's payload ends (q for k = 0)
  uint32_t next;     // the least avail at which more rows could be complete (T for k == rows)
};

// The state a caller keeps between the calls of the incremental prefix decode (himg_hip_prefix_state of
// include/himg_hip.h, field for field).
struct PfxState {
  uint32_t started;      // 0: a fresh state
  int32_t rows_done;     // k: block rows [0, k) are in the caller's picture
  uint32_t walk_pos;     // PfxRows::used of the walk that found k
  uint32_t avail_seen;   // the bytes present then
};

// Can `s` (started != 0) be the state a call at fewer or as many bytes left on this stream?  q: the first
// row header, end: the chunk's end (pfx_chain, pfx_tree_len).  Every field is judged before a load uses it.
__host__ __device__ inline bool pfx_state_ok(const PfxState &s, uint32_t avail, int rows, uint32_t q, uint32_t end) {
  return avail >= s.avail_seen && s.rows_done >= 0 && s.rows_done <= rows && s.walk_pos >= q && s.walk_pos <= end &&
         s.walk_pos <= avail;
}

// The row headers from `q` to the chunk's end, for as long as a header and its payload lie wholly below
// avail.  The walk stands at `q` = PfxRows::used of an earlier walk over fewer (or as many) bytes of the same
// stream, which found r0 complete rows (r0 = 0: q is the first header); row_off / row_len are written for
// rows [r0, k) only.  Where the chunk holds blocks behind the last block row, `used` stays at the last row's
// end and their headers are walked again by every call.
__host__ __device__ inline int pfx_rows_from(const uint8_t *p, uint32_t avail, uint32_t T, int fix_t2, int rows,
                                             uint32_t q, int r0, uint32_t end, uint32_t *row_off, uint32_t *row_len,
                                             PfxRows *out) {
  out->k = r0; out->used = q; out->next = T;
  if (fix_t2 && rows == 1) {   // the encoder writes one block row without a size header
    if (r0 == 0) {
      if (end <= avail) {
        out->k = 1; out->used = end;
        if (row_off) { row_off[0] = q; row_len[0] = end - q; }
      } else {
        out->next = end;
      }
    }
    return kPfxOk;
  }
  int r = r0;
  bool cut = false;
  while (q != end) {
    uint32_t b = 0, len = 0;
    const int rc = pfx_row_header(p, q, end, avail, &b, &len, &out->next);
    if (rc == kPfxFormat) return kPfxFormat;
    if (rc == kPfxShort) { cut = true; break; }
    if (r < rows) {
      if (row_off) { row_off[r] = b; row_len[r] = len; }
      out->used = b + len;
    }
    ++r;
    q = b + len;
  }
  if (!cut && r < rows) return kPfxFormat;   // fewer blocks than block rows
  out->k = r < rows ? r : rows;
  if (out->k == rows) out->next = T;
  return kPfxOk;
}

// The walk from the first row header.
__host__ __device__ inline int pfx_rows(const uint8_t *p, uint32_t avail, uint32_t T, int fix_t2, int rows, uint32_t q,
                                        uint32_t end, uint32_t *row_off, uint32_t *row_len, PfxRows *out) {
  return pfx_rows_from(p, avail, T, fix_t2, rows, q, 0, end, row_off, row_len, out);
}

}  // namespace himg_dev
#endif  // HIMG_PREFIX_WALK_H_
