// kernels_dec.hip -- HIMG decode path as hand-written HIP for gfx950 (MI355X).
//
// Pipeline (all on device, batched over frames):
//   k_dec_parse       RIFF chunk headers, mapping tables, QCFG, both Huffman trees,
//                     decode tables (decoder.cpp:144-290,428-461, huffman_dec.cpp:152-229)
//   k_dec_rowwalk     index of the FRES block rows (huffman_dec.cpp:232-248), side stream
//   k_lres_spec, k_lres_fix, k_lres_write, k_lres_finish
//                     the LRES stream, all chunks in parallel (huffman_dec.cpp:274-418)
//   k_lres_unpredict  inverse low-res prediction              (downsampled.cpp:318-382)
//   k_row_count       fixpoint rounds of every FRES block row (huffman_dec.cpp:274-418)
//   k_dec_row_fused   per block row: write pass into LDS, dequantise, inverse WHT,
//                     low-res add, clamp, colour inverse, pixel stores
//                     (decoder.cpp:331-426, quantize.cpp:153-165, hadamard.cpp:90-103,
//                     ycbcr.cpp:54-82)
//   k_dec_huff, k_tile_inv
//                     the same two steps through HBM for rows wider than the LDS, and
//                     the serial LRES fallback
//   k_dec_region, k_dec_scaled
//                     a rectangle at full resolution; the picture at 1/2 and 1/4 scale from each
//                     tile's lowest-sequency coefficients (no counterpart in the reference)
//   k_dec_row_fused_t, k_tile_inv_t, k_dec_region_t
//                     the tensor forms of the three kernels that write full-resolution pixels: a
//                     planar, normalised float32 / float16 / bfloat16 output converted in the store
//                     stage (TensDesc; include/himg_hip.h, "tensor decode")
//   k_dec_row_fused_p, k_tile_inv_p, k_dec_region_p
//                     their pitched forms: the same interleaved bytes at a row pitch, a pixel
//                     stride and an origin per frame (DstDesc; include/himg_hip.h, "decode into")
//   k_dec_row_fused_m, k_tile_inv_m
//                     the pyramid forms of the two row kernels: besides the full picture, the 1/2-
//                     and 1/4-scale ones from the same symbols (PyrDesc; include/himg_hip.h,
//                     "picture pyramid"; the 1/8-scale level is k_lres_preview's)
//   k_dec_row_fused_c, k_tile_inv_c
//                     their planes forms: the stream's own channel planes in front of the colour
//                     inverse, the wanted ones alone (PlaneDesc; include/himg_hip.h, "planes decode")
// One entropy-decode engine serves all of them: see "Entropy decoding" below.
#include "himg_dev.h"
#include "prefix_walk.h"
#include "loop_counts.h"

#include <cstdlib>
#include <type_traits>

namespace himg_dev {

__device__ static constexpr uint8_t kScanD[64] = {
    0,  1,  9,  8,  16, 17, 18, 10, 2,  3,  11, 19, 27, 26, 25, 24,
    32, 33, 34, 35, 36, 28, 20, 12, 4,  5,  13, 21, 29, 37, 45, 44,
    43, 42, 41, 40, 48, 49, 50, 51, 52, 53, 54, 46, 38, 30, 22, 14,
    6,  7,  15, 23, 31, 39, 47, 55, 63, 62, 61, 60, 59, 58, 57, 56};

// Inverse of kScanD: kInvScanD[row-major position] = index in the coefficient scan.
__device__ static constexpr uint8_t kInvScanD[64] = {
    0, 1, 8, 9, 24, 25, 48, 49, 3, 2, 7, 10, 23, 26, 47, 50, 4, 5, 6, 11, 22, 27, 46, 51, 15, 14, 13, 12, 21, 28, 45, 52, 16, 17, 18, 19, 20, 29, 44, 53, 35, 34, 33, 32, 31, 30, 43, 54, 36, 37, 38, 39, 40, 41, 42, 55, 63, 62, 61, 60, 59, 58, 57, 56};

// Device status values (host maps them to HIMG_ERR_*): 0 ok, 1 geometry
// mismatch, 3 outside the built scope, 4 the reference would return false.
// A format error also carries the decoder stage that failed in bits 4..7 and
// "the Huffman layer complained first" in bit 8, so that the C++ wrapper can
// print the same lines as the reference (decoder.cpp:96-135,232,287,345).
constexpr int kStGeom = 1, kStUnsupported = 3, kStFormat = 4;
__device__ __host__ constexpr int fmt_err(int stage, int huff) { return kStFormat | (stage << 4) | (huff << 8); }
constexpr int kMaxDepth = 32;   // deepest code the decoder walks (the reference encoder keeps codes in uint32_t)
constexpr int kMaxNodes = 2 * kNumSym - 1;
constexpr int kMaxSlow = 128;   // kLutBits-bit prefixes that get a second-level sub-table

__device__ __forceinline__ int clamp255d(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

__device__ __forceinline__ uint32_t rd32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Forward chunk search (decoder.cpp:428-461).  Returns false when not found.
__device__ bool find_chunk(const uint8_t *p, uint32_t n, uint32_t *idx, uint32_t tag,
                           uint32_t *size) {
  for (;;) {
    if (*idx + 8 > n) return false;
    const uint32_t t = rd32(p + *idx), sz = rd32(p + *idx + 4);
    *idx += 8;
    if (sz > 0x7fffffffu || (unsigned long long)*idx + sz > n) return false;
    if (t == tag) { *size = sz; return true; }
    *idx += sz;
  }
}

// Pre-order tree recovery (huffman_dec.cpp:152-213), in parallel.  The reference reads
// the serialised tree node by node (a branch is one 0 bit, a leaf a 1 bit and nine symbol
// bits); as a single-lane loop that is 250 instructions of divergent control per node
// and 120 us per frame.  Here:
//   A  where the nodes start.  One lane per 32-bit word runs the walk over its word
//      from each of the ten possible entry states (0..9 = bits of a leaf left over from
//      the previous word): exit state and node count per entry state.  One lane chains
//      the (at most 96) words; the word lanes then write their nodes' start bits.
//   B  the tree.  open[k] = stack depth of the reference's walk after node k (a prefix
//      sum of +1 / -1); the tree ends at the first node where it is 0.  A node that
//      follows a branch is its first child; one that follows a leaf is the second child
//      of the nearest earlier branch j with open[j] == open[k - 1] + 1 (the branch whose
//      pending child sat on top of the stack).  Depth and code (LSB = first choice)
//      follow from the parent links by pointer jumping.
// Per node the low bits of its code and its depth are kept in aux[] for the table
// fills; the nodes go to LDS in the packed form the tree walks read (child a |
// child b << 10 | (symbol + 1) << 20, 1023 = no child).
struct TreeAux { uint32_t code; int32_t depth; };

constexpr int kTreeWords = kTreeStride / 4;       // words of a staged serialised tree
constexpr int kNodeCap = kMaxNodes + 1;           // node slots (a tree of more nodes is rejected)
struct TreeScratch {                              // phases A / B of one tree
  unsigned long long outs[kTreeWords], cnts[kTreeWords];   // 4 / 6 bits per entry state
  uint32_t went[kTreeWords];                      // entry state | first node << 4
  uint16_t pos[kNodeCap + 6];                     // start bit | leaf << 15
  int16_t open[2][kNodeCap + 6];                  // prefix sums (two buffers)
  __attribute__((aligned(16))) int16_t key[kNodeCap + 14];   // open[] of branches, 0 for leaves
  uint16_t anc[kNodeCap + 6];
  uint16_t second[kNodeCap + 6];                  // second child of a branch
  int32_t total, first_bad, kend, kdeep;
};

// One entry of the LMAP / FMAP mapping table from bytes staged in LDS (mapper.cpp:127-157):
// entries 1..n1 are one byte each, the others two.
__device__ __forceinline__ bool map_ok(const uint8_t *in, uint32_t size) {
  return size >= 1 && in[0] <= 127 && (uint32_t)(1 + in[0] + 2 * (127 - in[0])) == size;
}
__device__ __forceinline__ int16_t map_entry(const uint8_t *in, int i) {
  const int n1 = in[0] <= 127 ? in[0] : 127;
  if (i == 0) return 0;
  if (i <= n1) return (int16_t)in[i];
  const uint8_t *q = in + 1 + n1 + 2 * (i - n1 - 1);
  return (int16_t)(uint16_t)(q[0] | (q[1] << 8));
}

// LUT entry: [8:0] symbol | [9] "continue at node" flag | [15:10] code bits |
// [19:16] RLE extra bits of the symbol | [31:20] node index (the leaf itself, or
// for flagged entries the branch reached after kLutBits bits).
__device__ __forceinline__ int rle_extra_bits(int sym) {
  return sym < 257 ? 0 : sym == 257 ? 2 : sym == 258 ? 4 : sym == 259 ? 8 : 14;
}
__device__ __forceinline__ uint32_t lut_leaf(int sym, int bits) {
  return (uint32_t)sym | ((uint32_t)bits << 10) | ((uint32_t)rle_extra_bits(sym) << 16);
}
__device__ __forceinline__ uint32_t lut_node(int node, int bits) {
  return 512u | ((uint32_t)bits << 10) | ((uint32_t)node << 20);
}
// Step word of the decoder (see "Entropy decoding" below): [4:0] code bits to
// consume, [9:5] extra bits that follow, [18:10] symbols produced before the
// extra-bits value is added, [22:19] code bits / [25:23] class of the group's first
// token, [31:27] = [4:0] + [9:5].
__device__ __forceinline__ uint32_t grp_y(uint32_t tb, uint32_t eb, uint32_t cb, uint32_t s_tb, uint32_t s_class) {
  return tb | (eb << 5) | (cb << 10) | (s_tb << 19) | (s_class << 23) | ((tb + eb) << 27);
}
// Second-level entry of a token whose code is longer than kLutBits (the first
// kLutBits bits are consumed before it is read): [4:0] the remaining code bits (>= 1,
// which tells it from a node reference), [9:5] extra bits, [18:10] run base / 1,
// [26:19] the literal byte.
__device__ __forceinline__ uint32_t sub_leaf(int sym, uint32_t rest_bits) {
  const uint32_t c = sym < 256 ? 0u : (uint32_t)sym - 255u;
  const uint32_t eb = (0xE84200u >> (4u * c)) & 15u;
  const unsigned long long kBases = 1ull | (2ull << 9) | (3ull << 18) | (7ull << 27) | (23ull << 36) | (279ull << 45);
  const uint32_t cb = (uint32_t)(kBases >> (9u * c)) & 511u;
  return rest_bits | (eb << 5) | (cb << 10) | ((sym < 256 ? (uint32_t)sym : 0u) << 19);
}

// ---------------------------------------------------------------------------
// k_dec_parse: one 1024-thread workgroup per frame.
//   1. thread 0 walks the chunk headers only (decoder.cpp:144-290): RIFF, FRMT,
//      LMAP, LRES, QCFG, FMAP, FRES -- a chain of dependent global reads;
//   2. the workgroup stages the small bodies (mapping tables, QCFG, the two
//      serialised trees) in LDS, all five in one round of loads;
//   3. the two trees are recovered side by side (512 lanes each, see "Pre-order tree
//      recovery" above); lanes 128..415 parse the tables;
//   4. the verdict is the FIRST failure in the reference's order of checks;
//   5. the decode tables of BOTH streams are built side by side, 512 lanes each.
// ---------------------------------------------------------------------------
// HEAD (k_dec_parse_head, the 1/8-scale preview): only what the reference checks in front of
// QCFG (decoder.cpp:95-118) -- the headers RIFF .. LRES, the LMAP body, the LRES tree and its
// decode tables; head_sizes[f] receives the byte offset of the end of the LRES chunk (the
// packed size where it was not found), the bound the LRES kernels' readers are given.
constexpr int kParseThreads = 1024;
constexpr int kParseHalf = kParseThreads / 2;   // lanes per stream in step 5
__device__ __forceinline__ void identity_test_words(const DecFrame *df, int l, uint32_t *dst);

// PREFIX (k_dec_parse_prefix, the decode of a stream prefix): sizes[f] is the size the stream's RIFF
// header declares, the container's bound; avails[f] the bytes present, below which k_span_gate has
// found every header this walk reads -- the staging of the bodies is bounded there.
template <bool HEAD, bool PREFIX = false>
__device__ __forceinline__ void dec_parse_body(Geom g, DecWs ws, const uint8_t *packed,
                                               size_t in_stride, const uint32_t *sizes, uint32_t *head_sizes,
                                               const uint32_t *avails = nullptr) {
  __shared__ TreeAux aux[2][kMaxNodes + 1];
  __shared__ uint32_t s_nd[2][kMaxNodes + 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_lut[2][1 << kLutBits];
  __shared__ uint32_t s_sub[2][kSubEntries];
  __shared__ __attribute__((aligned(16))) uint16_t s_heap[2][2 << kLutBits];
  __shared__ uint16_t s_symd[2][kMaxNodes + 1];
  __shared__ uint32_t s_nslow[2], s_slow_m[2][kMaxSlow], s_slow_off[2][kMaxSlow];
  // Staged chunk bodies: 0 LMAP, 1 LRES tree, 2 QCFG, 3 FMAP, 4 FRES tree.
  constexpr int kBodyBytes = kTreeStride + 16;
  __shared__ uint32_t s_buf[5][kBodyBytes / 4];
  __shared__ uint32_t s_off[5], s_sz[5];
  __shared__ int32_t s_nn[2];
  static_assert(sizeof(TreeScratch) <= sizeof(s_heap) && sizeof(TreeScratch) <= sizeof(s_lut),
                "the trees' scratch lives in the memory of the heap and the LUTs (unused until step 5)");
  // Verdict per check, in the reference's order (0 = passed / not reached).
  enum { cHead = 0, cLmap, cLresFind, cLresTree, cQcfg, cFmapFind, cFmap, cFresFind, cFresTree, cLeaf0, cLeaf1, cCount };
  __shared__ int s_chk[cCount];
  __shared__ int s_status;
  const int f = blockIdx.x, lane = threadIdx.x;   // lane = thread index in the workgroup
  const long long c_in = clock64();
  const uint8_t *p = packed + (size_t)f * in_stride;
  const uint32_t n = sizes[f];
  DecFrame *df = ws.frames + f;

  if (lane < cCount) s_chk[lane] = 0;
  if (lane < 5) { s_off[lane] = 0; s_sz[lane] = 0; }
  if (lane < 2) s_nn[lane] = 0;
  __syncthreads();

  if (lane == 0) {   // ---- 1: chunk headers, in file order
    uint32_t idx = 12, sz = 0;
    if (HEAD) df->walk_status = 0;   // (no row walk: k_dec_status reads the parse's verdict alone)
    do {
      if (n < 12 || rd32(p) != 0x46464952u /*RIFF*/ || rd32(p + 4) + 8u != n ||
          rd32(p + 8) != 0x474d4948u /*HIMG*/) { s_chk[cHead] = fmt_err(1, 0); break; }
      if (!find_chunk(p, n, &idx, 0x544d5246u /*FRMT*/, &sz) || sz < 11 || p[idx] != 1) { s_chk[cHead] = fmt_err(2, 0); break; }
      const uint32_t w = rd32(p + idx + 1), h = rd32(p + idx + 5);
      const int c = p[idx + 9];
      df->ycbcr = (p[idx + 10] != 0 && c >= 3) ? 1 : 0;
      if ((int)w != g.W || (int)h != g.H || c != g.C) { s_chk[cHead] = kStGeom; break; }
      idx += sz;
      if (!find_chunk(p, n, &idx, 0x50414d4cu /*LMAP*/, &sz)) { s_chk[cHead] = fmt_err(3, 0); break; }
      s_off[0] = idx; s_sz[0] = sz;
      idx += sz;
      if (!find_chunk(p, n, &idx, 0x5345524cu /*LRES*/, &sz)) { s_chk[cLresFind] = fmt_err(4, 0); break; }
      df->s[0].chunk_end = idx + sz;
      s_off[1] = idx; s_sz[1] = sz;
      if (HEAD) break;
      idx += sz;
      if (!find_chunk(p, n, &idx, 0x47464351u /*QCFG*/, &sz) || sz != (df->ycbcr ? 64u : 32u)) { s_chk[cQcfg] = fmt_err(5, 0); break; }
      s_off[2] = idx; s_sz[2] = sz;
      idx += sz;
      if (!find_chunk(p, n, &idx, 0x50414d46u /*FMAP*/, &sz)) { s_chk[cFmapFind] = fmt_err(6, 0); break; }
      s_off[3] = idx; s_sz[3] = sz;
      idx += sz;
      if (!find_chunk(p, n, &idx, 0x53455246u /*FRES*/, &sz)) { s_chk[cFresFind] = fmt_err(7, 0); break; }
      df->s[1].chunk_end = idx + sz;
      // Trap T2: the decoder derives use_blocks from the COMPRESSED size
      // (huffman_dec.cpp:215-219); UncompressBlock refuses when it is false (:265).
      // (The opt-in fixed mode derives use_blocks like the encoder does: rows > 1.)
      if (!g.fix_t2 && !((uint32_t)g.row_block < sz)) { s_chk[cFresFind] = fmt_err(7, 1); break; }
      s_off[4] = idx; s_sz[4] = sz;
    } while (0);
    if (HEAD) head_sizes[f] = s_off[1] ? df->s[0].chunk_end : n;
  }
  __syncthreads();

  // ---- 2: stage the bodies (a dependent global load costs ~1 us, an LDS read ~50 ns)
  // (HEAD: LMAP and the LRES tree; the FRES side below finds no tree and recovers nothing.)
  for (int k = lane; k < (HEAD ? 2 : 5) * kBodyBytes; k += kParseThreads) {
    const int b = k / kBodyBytes, j = k - b * kBodyBytes;
    uint32_t cnt = s_sz[b] < (uint32_t)kTreeStride ? s_sz[b] : (uint32_t)kTreeStride;
    if constexpr (PREFIX) {   // (the FRES tree's 384 bytes may reach into rows that have not arrived)
      const uint32_t av = avails[f], left = av > s_off[b] ? av - s_off[b] : 0u;
      cnt = cnt < left ? cnt : left;
    }
    reinterpret_cast<uint8_t *>(s_buf[b])[j] = (uint32_t)j < cnt ? p[s_off[b] + j] : (uint8_t)0;
  }
  __syncthreads();

  // ---- 3: the two trees side by side, 512 lanes each: LRES (decoder.cpp:232) and FRES
  // (decoder.cpp:290), huffman_dec.cpp:152-229
  {
    const int s = lane / kParseHalf, l = lane - s * kParseHalf, b = s ? 4 : 1;
    TreeScratch *ts = s ? reinterpret_cast<TreeScratch *>(&s_lut[0][0]) : reinterpret_cast<TreeScratch *>(&s_heap[0][0]);
    const uint32_t *w = s_buf[b];
    const bool present = s_off[b] != 0;
    const uint32_t nbytes = !present ? 0u : s_sz[b] < (uint32_t)kTreeStride ? s_sz[b] : (uint32_t)kTreeStride;
    const uint32_t bit_end = 8u * nbytes;
    const int nw = (int)((bit_end + 31u) >> 5);
    // A1: the walk over one word from every entry state
    if (l < nw) {
      const uint32_t x = w[l];
      unsigned long long outs = 0, cnts = 0;
      for (uint32_t e = 0; e < 10; ++e) {
        uint32_t pos = e, c = 0;
        while (pos < 32u) { ++c; pos += ((x >> pos) & 1u) ? 10u : 1u; }
        outs |= (unsigned long long)(pos - 32u) << (4u * e);
        cnts |= (unsigned long long)c << (6u * e);
      }
      ts->outs[l] = outs; ts->cnts[l] = cnts;
    }
    if (l == 0) { ts->first_bad = kNodeCap; ts->kend = kNodeCap; ts->kdeep = kNodeCap; }
    for (int k = l; k < kNodeCap + 6; k += kParseHalf) { ts->second[k] = 0; ts->key[k] = 0; }
    __syncthreads();
    // A2: chain the words
    if (l == 0) {
      uint32_t state = 0, base = 0;
      for (int k = 0; k < nw; ++k) {
        ts->went[k] = state | (base << 4);
        base += (uint32_t)(ts->cnts[k] >> (6u * state)) & 63u;
        state = (uint32_t)(ts->outs[k] >> (4u * state)) & 15u;
      }
      ts->total = (int32_t)(base < (uint32_t)kNodeCap ? base : (uint32_t)kNodeCap);
    }
    __syncthreads();
    // A3: the nodes' start bits
    if (l < nw) {
      const uint32_t x = w[l], e = ts->went[l] & 15u;
      uint32_t k = ts->went[l] >> 4, pos = e;
      while (pos < 32u && k < (uint32_t)kNodeCap) {
        const uint32_t leaf = (x >> pos) & 1u;
        ts->pos[k++] = (uint16_t)((32u * (uint32_t)l + pos) | (leaf << 15));
        pos += leaf ? 10u : 1u;
      }
    }
    __syncthreads();
    // B1: open[] and where the tree ends
    const int total = ts->total;
    for (int k = l; k < kNodeCap; k += kParseHalf) {
      int16_t d = 0;
      if (k < total) {
        const uint32_t pp = ts->pos[k], leaf = pp >> 15, bp = pp & 0x7fffu;
        d = leaf ? (int16_t)-1 : (int16_t)1;
        // ReadBitChecked / ReadBitsChecked, huffman_dec.cpp:51-60, 94-106
        if (bp >= bit_end || (leaf && bp + 10u > bit_end)) atomicMin(&ts->first_bad, k);
      }
      ts->open[0][k] = d;
    }
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kNodeCap; d <<= 1) {
      for (int k = l; k < kNodeCap; k += kParseHalf)
        ts->open[cur ^ 1][k] = (int16_t)(ts->open[cur][k] + (k >= d ? ts->open[cur][k - d] : 0));
      cur ^= 1;
      __syncthreads();
    }
    const int16_t *open = ts->open[cur];   // (stack depth after node k) - 1
    for (int k = l; k < total; k += kParseHalf) {
      if (open[k] == -1) atomicMin(&ts->kend, k);
      if (!(ts->pos[k] >> 15)) ts->key[k] = (int16_t)(open[k] + 1);   // >= 2 for a branch
    }
    __syncthreads();
    // The first node the reference's walk fails on (count >= kMaxNodes, or the bits run
    // out: huffman_dec.cpp:51-60), if any.
    const int kend = ts->kend, first_bad = ts->first_bad;
    const bool whole = kend < kMaxNodes && first_bad > kend;
    const int ka = whole ? kNodeCap : min(min(first_bad, total), kMaxNodes);
    const int nlim = whole ? kend + 1 : ka;   // nodes the walk has read
    // B2: parents
    for (int k = l; k < nlim; k += kParseHalf) {
      int par = 0, which = 0;
      if (k > 0) {
        if (!(ts->pos[k - 1] >> 15)) {
          par = k - 1;
        } else {
          which = 1;
          const uint32_t t = (uint32_t)(uint16_t)(open[k - 1] + 2), tt = t | (t << 16);
          const int j0 = k - 2;
          int found = -1;
          for (int c = j0 >> 3; c >= 0 && found < 0; --c) {
            const uint4 q = *reinterpret_cast<const uint4 *>(&ts->key[8 * c]);
            const uint32_t xs[4] = {q.x ^ tt, q.y ^ tt, q.z ^ tt, q.w ^ tt};
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) any |= (xs[i] - 0x00010001u) & ~xs[i] & 0x80008000u;
            if (!any) continue;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const int idx = 8 * c + i;
              if (idx <= j0 && ((xs[i >> 1] >> (16 * (i & 1))) & 0xffffu) == 0u) found = idx;
            }
          }
          par = found < 0 ? 0 : found;
          ts->second[par] = (uint16_t)k;
        }
      }
      ts->anc[k] = (uint16_t)par;
      TreeAux a; a.code = (uint32_t)which; a.depth = k > 0 ? 1 : 0;
      aux[s][k] = a;
    }
    __syncthreads();
    // B3: depth and code by pointer jumping (a depth beyond 63 stays at >= 32: rejected below)
    for (int r = 0; r < 6; ++r) {
      static_assert(kNodeCap <= 2 * kParseHalf, "two nodes per lane");
      const int k0 = l, k1 = l + kParseHalf;
      TreeAux n0, n1;
      uint16_t a0 = 0, a1 = 0;
      n0.code = n1.code = 0; n0.depth = n1.depth = 0;
      if (k0 < nlim) {
        const int a = ts->anc[k0];
        const TreeAux me = aux[s][k0], up = aux[s][a];
        n0.code = up.code | (up.depth < 32 ? me.code << up.depth : 0u);
        n0.depth = min(me.depth + up.depth, 255);
        a0 = ts->anc[a];
      }
      if (k1 < nlim) {
        const int a = ts->anc[k1];
        const TreeAux me = aux[s][k1], up = aux[s][a];
        n1.code = up.code | (up.depth < 32 ? me.code << up.depth : 0u);
        n1.depth = min(me.depth + up.depth, 255);
        a1 = ts->anc[a];
      }
      __syncthreads();
      if (k0 < nlim) { aux[s][k0] = n0; ts->anc[k0] = a0; }
      if (k1 < nlim) { aux[s][k1] = n1; ts->anc[k1] = a1; }
      __syncthreads();
    }
    // B4: a branch deeper than the decoder walks; the packed nodes
    for (int k = l; k < nlim; k += kParseHalf) {
      const uint32_t pp = ts->pos[k], leaf = pp >> 15;
      if (!leaf) {
        if (aux[s][k].depth + 1 > kMaxDepth) atomicMin(&ts->kdeep, k);
        s_nd[s][k] = ((uint32_t)(k + 1) & 1023u) | ((uint32_t)ts->second[k] << 10);
      } else {
        const uint32_t bp = (pp & 0x7fffu) + 1u, wi = bp >> 5;
        const uint32_t sym = (uint32_t)((((unsigned long long)w[wi + 1] << 32) | w[wi]) >> (bp & 31u)) & 511u;
        s_nd[s][k] = 0xfffffu | ((sym + 1u) << 20);
      }
    }
    __syncthreads();
    if (l == 0 && present) {
      // The first failure in the order of the reference's walk.
      int st = 0;
      if (ts->kdeep < ka) st = kStUnsupported;
      else if (!whole) st = fmt_err(s ? 7 : 4, 1);
      if (!st) {
        const int nn = kend + 1;
        const uint32_t tb = ((ts->pos[kend] & 0x7fffu) + 10u + 7u) >> 3;   // AlignToByte, huffman_dec.cpp:229
        df->s[s].num_nodes = nn;
        s_nn[s] = nn;
        df->s[s].root = 0;
        df->s[s].payload_off = s_off[b] + tb;
        // UncompressStream's first test (huffman_dec.cpp:277-278): nothing left after the tree.
        if (df->s[s].payload_off >= df->s[s].chunk_end) st = fmt_err(s ? 7 : 4, 1);
        // A tree that is a single leaf decodes without consuming code bits in the
        // reference (huffman_dec.cpp:173-185 with bits == 0) and cannot round-trip
        // the encoder's 1-bit codes; such streams are rejected.
        // (Fixed mode: read them as the 1-bit codes the encoder writes, huffman_enc.cpp:231-237.)
        if (!st && nn == 1 && !g.fix_t2) s_chk[s ? cLeaf1 : cLeaf0] = fmt_err(s ? 7 : 4, 1);
      }
      s_chk[s ? cFresTree : cLresTree] = st;
    }
  }
  if (lane >= 128 && lane < 384) {       // mapping tables: one entry per lane
    const int m = (lane - 128) >> 7, i = (lane - 128) & 127, b = m ? 3 : 0;
    if (s_off[b]) {
      const uint8_t *in = reinterpret_cast<const uint8_t *>(s_buf[b]);
      const bool ok = s_sz[b] <= (uint32_t)kTreeStride && map_ok(in, s_sz[b]);
      if (ok) (m ? df->fmap : df->lmap)[i] = map_entry(in, i);
      else if (i == 0) s_chk[m ? cFmap : cLmap] = fmt_err(m ? 6 : 3, 0);
    }
  } else if (lane >= 384 && lane < 416) {   // QCFG, quantize.cpp:190-213
    if (s_off[2]) {
      const uint8_t *q = reinterpret_cast<const uint8_t *>(s_buf[2]);
      const int i = lane - 384;
      df->shift[0][2 * i] = q[i] >> 4; df->shift[0][2 * i + 1] = q[i] & 15;
      const uint8_t x = df->ycbcr ? q[32 + i] : 0;
      df->shift[1][2 * i] = x >> 4; df->shift[1][2 * i + 1] = x & 15;
    }
  }
  __syncthreads();
  if (lane == 0) {   // ---- 4: first failure in the reference's order
    int st = 0;
    for (int k = 0; k < cCount && !st; ++k) st = s_chk[k];
    s_status = st;
    df->status = st;
    df->parse_status = st;
  }
  __syncthreads();
  if (s_status) return;
  // The row kernels' tables (DecFrame::row_tabs).  df->fmap / df->shift were written by other
  // lanes of this workgroup in front of the two barriers above.
  if (!HEAD) {
    int16_t *um = reinterpret_cast<int16_t *>(df->row_tabs);
    uint8_t *sh = reinterpret_cast<uint8_t *>(df->row_tabs + 128);
    uint32_t *sp = df->row_tabs + 160;
    if (lane < 256) {
      const int sc = (int8_t)lane;
      um[lane] = (int16_t)(sc >= 0 ? df->fmap[sc] : (sc == -128 ? -df->fmap[127] : -df->fmap[-sc]));
    } else if (lane < 384) {
      sh[lane - 256] = df->shift[(lane - 256) >> 6][(lane - 256) & 63];
    } else if (lane < 448) {
      // The same shifts as packed pairs in tile_plane's register order.
      const int t = lane - 384, ch = t >> 5, e = t & 31, x = e >> 2, j = e & 3;
      sp[t] = (uint32_t)df->shift[ch][(2 * j) * 8 + x] | ((uint32_t)df->shift[ch][(2 * j + 1) * 8 + x] << 16);
    } else if (lane < 512) {
      identity_test_words(df, lane - 448, sp + 64);
    }
  }
  const long long c_serial = clock64();

  // ---- 5: both streams side by side (HEAD: the LRES stream's; the other half of the
  // workgroup only keeps the barriers)
  const int s = lane / kParseHalf, l = lane - s * kParseHalf;
  const int nn = s_nn[s];
  const int lut_n = (HEAD && s) ? 0 : (1 << kLutBits), sub_n = (HEAD && s) ? 0 : kSubEntries;
  // The packed nodes, for the tree walks of the row kernels (codes longer than both tables).
  {
    uint32_t *nodes = ws.nodes + ((size_t)f * 2 + s) * (kMaxNodes + 1);
    for (int k = l; k < nn; k += kParseHalf) nodes[k] = s_nd[s][k];
  }
  // First-level LUTs (kLutBits wide, LSB-first codes index them directly) in LDS,
  // then the group tables derived from them.  Every node of depth <= kLutBits is
  // first entered in an implicit heap (index (1 << depth) | code); an entry then
  // finds its leaf with at most kLutBits independent reads instead of every leaf
  // replicating itself (a depth-1 leaf would write half the table on one lane).
  static_assert(sizeof(s_heap) == 16 * kParseThreads, "one 16-byte store per lane");
  reinterpret_cast<uint4 *>(&s_heap[0][0])[lane] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  for (int k = l; k < nn; k += kParseHalf) {
    const int depth = aux[s][k].depth;
    if (depth > kLutBits) continue;
    const int sym = (int)(s_nd[s][k] >> 20) - 1;
    // leaf: k + 1; branch (only looked at on the last level): 0x8000 | k
    s_heap[s][(1u << depth) | aux[s][k].code] = (uint16_t)(sym >= 0 ? k + 1 : (0x8000 | k));
    s_symd[s][k] = (uint16_t)(sym >= 0 ? sym : 0x8000);
  }
  __syncthreads();
  for (uint32_t idx = l; idx < (uint32_t)lut_n; idx += kParseHalf) {
    uint32_t e = 0;
    // depth 0: a tree that is one leaf (rejected above, kept consistent anyway)
    uint32_t h = s_heap[s][1];
    if (h && !(h & 0x8000u)) e = lut_leaf(s_symd[s][h - 1], g.fix_t2 ? 1 : 0) | ((h - 1) << 20);
    for (int d = 1; d <= kLutBits && !e; ++d) {
      h = s_heap[s][(1u << d) | (idx & ((1u << d) - 1u))];
      if (h && !(h & 0x8000u)) e = lut_leaf(s_symd[s][h - 1], d) | ((h - 1) << 20);
      else if (h && d == kLutBits) e = lut_node(h & 0x7fffu, d);
    }
    s_lut[s][idx] = e;
  }
  if (l == 0) s_nslow[s] = 0;
  for (int k = l; k < sub_n; k += kParseHalf) s_sub[s][k] = 0;
  __syncthreads();
  const long long c_lut = clock64();
  // Second-level tables for codes longer than kLutBits.  Few kLutBits-bit prefixes
  // lead to such codes; each gets a sub-table indexed by the next m bits (m = the
  // deepest leaf below it, at most kSubMaxBits; deeper leaves continue from a
  // branch node).  The flagged first-level entry keeps its slot in bits [8:0].
  for (uint32_t idx = l; idx < (uint32_t)lut_n; idx += kParseHalf) {
    const uint32_t e = s_lut[s][idx];
    if (e & 512u) {
      const uint32_t slot = atomicAdd(&s_nslow[s], 1u);
      s_lut[s][idx] = e | (slot < (uint32_t)kMaxSlow ? slot : 511u);
      if (slot < (uint32_t)kMaxSlow) s_slow_m[s][slot] = 0;
    }
  }
  __syncthreads();
  for (int k = l; k < nn; k += kParseHalf) {
    const int depth = aux[s][k].depth;
    if ((s_nd[s][k] >> 20) != 0 && depth > kLutBits) {
      const uint32_t slot = s_lut[s][aux[s][k].code & ((1u << kLutBits) - 1)] & 511u;
      if (slot < (uint32_t)kMaxSlow) atomicMax(&s_slow_m[s][slot], (uint32_t)(depth - kLutBits));
    }
  }
  __syncthreads();
  if (l == 0) {
    const uint32_t ns = s_nslow[s] < (uint32_t)kMaxSlow ? s_nslow[s] : (uint32_t)kMaxSlow;
    uint32_t off = 0;
    for (uint32_t q = 0; q < ns; ++q) {
      uint32_t m = s_slow_m[s][q] < (uint32_t)kSubMaxBits ? s_slow_m[s][q] : (uint32_t)kSubMaxBits;
      if (off + (1u << m) > (uint32_t)kSubEntries) m = 0;   // no room: plain tree walk
      s_slow_m[s][q] = m;
      s_slow_off[s][q] = off;
      if (m) off += 1u << m;
    }
  }
  __syncthreads();
  for (int k = l; k < nn; k += kParseHalf) {
    const int depth = aux[s][k].depth;
    if (depth <= kLutBits) continue;
    const uint32_t code = aux[s][k].code;
    const uint32_t slot = s_lut[s][code & ((1u << kLutBits) - 1)] & 511u;
    if (slot >= (uint32_t)kMaxSlow) continue;
    const uint32_t m = s_slow_m[s][slot], off = s_slow_off[s][slot];
    const uint32_t d = (uint32_t)(depth - kLutBits), rel = code >> kLutBits;
    const int sym = (int)(s_nd[s][k] >> 20) - 1;
    if (m == 0 || d > m) continue;
    if (sym >= 0) {
      // A valid leaf: the token resolved in the decoder's step format.  A symbol the
      // reference rejects stays a node reference: the walk ends on it and flags it.
      const uint32_t e = sym <= 260 ? sub_leaf(sym, d) : lut_node(k, depth);
      for (uint32_t i = 0; i < (1u << (m - d)); ++i) s_sub[s][off + ((i << d) | rel)] = e;
    } else if (d == m) {
      s_sub[s][off + rel] = lut_node(k, depth);
    }
  }
  __syncthreads();
  {
    // Out in the decoder's entry form: .x the literal byte, .y the step word of the ONE
    // token (code bits = what is left of the code after the kLutBits-bit prefix); a node
    // reference as .x = node | depth << 16, .y = 0 (also "nothing there": 0, 0).
    uint2 *sub = ws.sub + ((size_t)f * 2 + s) * kSubEntries;
    for (int k = l; k < sub_n; k += kParseHalf) {
      const uint32_t e = s_sub[s][k];
      uint2 o;
      if (e & 31u) {
        const uint32_t rest = e & 31u, eb = (e >> 5) & 31u, cb = (e >> 10) & 511u;
        const uint32_t cls = eb == 0 ? (cb == 2 ? 1u : 0u) : (eb == 2 ? 2u : eb == 4 ? 3u : eb == 8 ? 4u : 5u);
        o.x = (e >> 19) & 255u;
        o.y = grp_y(rest, eb, cb, rest, cls);
      } else {
        o.x = (e >> 20) | (((e >> 10) & 63u) << 16);
        o.y = 0;
      }
      sub[k] = o;
    }
  }
  const long long c_sub = clock64();
  {
    // Group table of the lean decoder (GrpTables below).  A group is a greedy
    // sequence of tokens whose CODES lie inside the kLutBits known bits:
    // literals / single zeros / the two-zeros symbol for at most 4 output bytes,
    // optionally closed by ONE zero-run token (its zeros need no explicit bytes;
    // its extra bits are read from the stream at decode time).
    uint2 *grp = ws.grp + ((size_t)f * 2 + s) * (1u << kLutBits);
    for (uint32_t idx = l; idx < (uint32_t)lut_n; idx += kParseHalf) {
      uint32_t used = 0, nout = 0, bytes = 0, g_eb = 0, s_tb = 0, s_class = 0, ntok = 0;
      const uint32_t e0 = s_lut[s][idx];
      for (;;) {
        const uint32_t e = s_lut[s][(idx >> used) & ((1u << kLutBits) - 1)];
        const uint32_t len = (e >> 10) & 63u, sym = e & 511u;
        if ((e & 512u) || len == 0 || sym > 260 || used + len > (uint32_t)kLutBits) break;
        uint32_t cls;
        if (sym <= 256) {
          const uint32_t cnt = sym == 256 ? 2u : 1u;
          if (nout + cnt > 4) break;
          if (sym < 256) bytes |= sym << (8 * nout);
          nout += cnt;
          cls = sym == 256 ? 1u : 0u;
        } else {
          cls = sym - 255u;  // 2..5
          nout += cls == 2 ? 3u : cls == 3 ? 7u : cls == 4 ? 23u : 279u;
          g_eb = cls == 2 ? 2u : cls == 3 ? 4u : cls == 4 ? 8u : 14u;
        }
        used += len;
        if (ntok++ == 0) { s_tb = len; s_class = cls; }
        if (sym > 256) break;
      }
      uint2 r;
      if (ntok) {
        r.x = bytes;
        r.y = grp_y(used, g_eb, nout, s_tb, s_class);
      } else {
        // The first code is longer than the table: .x says where to continue --
        // bit 31 set: sub-table (offset << 8 | index bits); else the tree walk
        // from node | depth << 16.
        const uint32_t slot = e0 & 511u;
        if ((e0 & 512u) && slot < (uint32_t)kMaxSlow && s_slow_m[s][slot])
          r.x = 0x80000000u | (s_slow_off[s][slot] << 8) | s_slow_m[s][slot];
        else
          r.x = (e0 >> 20) | (((e0 >> 10) & 63u) << 16);
        r.y = 0;
      }
      grp[idx] = r;
      // The same greedy group WITHOUT the four-byte limit, for the passes that only
      // count (k_row_count, lead-ins): as many tokens as have their codes inside the
      // kLutBits known bits -- more bits per step where zeros and short literals
      // alternate.
      uint32_t yc = 0;
      if (ntok) {
        uint32_t u2 = 0, n2 = 0, eb2 = 0;
        for (;;) {
          const uint32_t e = s_lut[s][(idx >> u2) & ((1u << kLutBits) - 1)];
          const uint32_t len = (e >> 10) & 63u, sym = e & 511u;
          if ((e & 512u) || len == 0 || sym > 260 || u2 + len > (uint32_t)kLutBits) break;
          u2 += len;
          if (sym <= 256) { n2 += sym == 256 ? 2u : 1u; continue; }
          const uint32_t cls = sym - 255u;
          n2 += cls == 2 ? 3u : cls == 3 ? 7u : cls == 4 ? 23u : 279u;
          eb2 = cls == 2 ? 2u : cls == 3 ? 4u : cls == 4 ? 8u : 14u;
          break;
        }
        yc = grp_y(u2, eb2, n2, s_tb, s_class);
      }
      ws.gyc[((size_t)f * 2 + s) * (1u << kLutBits) + idx] = yc;
    }
  }
  if (!HEAD && lane == 0) {   // phase cycles / 16 for tools/dec_stats.py (after the memset of stats)
    uint32_t *st = ws.parse_stats + (size_t)f * 4;
    st[0] = (uint32_t)((c_serial - c_in) >> 4); st[1] = (uint32_t)((c_lut - c_serial) >> 4);
    st[2] = (uint32_t)((c_sub - c_lut) >> 4); st[3] = (uint32_t)((clock64() - c_sub) >> 4);
  }
}

__global__ __launch_bounds__(kParseThreads) void k_dec_parse(Geom g, DecWs ws, const uint8_t *packed,
                                                             size_t in_stride, const uint32_t *sizes) {
  dec_parse_body<false>(g, ws, packed, in_stride, sizes, nullptr);
}

__global__ __launch_bounds__(kParseThreads) void k_dec_parse_head(Geom g, DecWs ws, const uint8_t *packed,
                                                                  size_t in_stride, const uint32_t *sizes,
                                                                  uint32_t *head_sizes) {
  dec_parse_body<true>(g, ws, packed, in_stride, sizes, head_sizes);
}

__global__ __launch_bounds__(kParseThreads) void k_dec_parse_prefix(Geom g, DecWs ws, const uint8_t *packed,
                                                                    size_t in_stride, const uint32_t *sizes,
                                                                    const uint32_t *avails) {
  dec_parse_body<false, true>(g, ws, packed, in_stride, sizes, nullptr, avails);
}

// ---------------------------------------------------------------------------
// k_dec_rowwalk: index of the FRES block rows (huffman_dec.cpp:232-248).  Every
// row's size header sits right behind the previous row's payload, so this is a
// chain of dependent loads (0.45 us per hop for 4096-pixel rows, 0.64 us for
// 16384-pixel ones) that nothing can parallelise; it runs on a side stream, beside
// k_dec_parse and the LRES kernels.  (Tried and dropped, profiles/r03_experiments.md:
// other waves of the workgroup touching the chunk a bounded distance ahead so that the
// hops hit in L2 -- slower; the headers through the scalar cache -- 9 % faster at
// 4096 pixels, 38 % slower at 16384.)
// ---------------------------------------------------------------------------
// A single frame's walk is cut into row ranges, one launch each (row_end: walk the rows in
// front of it; the last launch walks to the end of the chunk; resume: continue where the
// launch before stopped, DecFrame::walk_q / walk_r): the counts and the row kernels of a
// range run while the next range is walked (launch_decode).  The body (dec_body_rowwalk.inc) is
// also the region decode's per-frame form's, k_region_rowwalk.
__global__ __launch_bounds__(64) void k_dec_rowwalk(Geom g, DecWs ws, const uint8_t *packed,
                                                    size_t in_stride, const uint32_t *sizes,
                                                    int row_end, int resume) {
#include "dec_body_rowwalk.inc"
}

// k_dec_set_index: the row index comes from the caller (row-sharded decode: the rank
// that holds the whole stream walked the headers once, the others hold only their own
// rows' bytes and cannot) -- [rows] payload offsets, then [rows] lengths.  Rows whose
// payload would leave the stream are flagged like a damaged header.  The body (dec_body_set_index.inc)
// is also the region decode's per-frame form's, k_region_set_index.
__global__ __launch_bounds__(256) void k_dec_set_index(Geom g, DecWs ws, const uint32_t *index,
                                                       const uint32_t *sizes, int r0, int r1) {
#include "dec_body_set_index.inc"
}

// ---------------------------------------------------------------------------
// Entropy decoding (huffman_dec.cpp:274-418), parallel inside one stream.
//
// A whole workgroup (1024 lanes) decodes one Huffman stream (the LRES stream or
// one FRES block row).  The payload is processed in chunks of 1024 sub-sequences.
// Every lane decodes one sub-sequence speculatively from its nominal start; then
// the workgroup iterates start[t+1] = end[t] until nothing changes.  Lane 0's
// start is exact, so by induction the fixpoint is the exact token chain (Huffman
// streams self-synchronise, typically within one sub-sequence).  A prefix scan
// of the per-lane symbol counts places the output, and a last pass writes it.
//
// These passes are bound by VALU issue (a CU retires one wave64 VALU
// instruction per cycle), so the inner loop is kept to a few dozen instructions
// per step: a 64-bit bit window per lane over the payload in place (L2), ONE
// table read per step that resolves a whole group of tokens, and no per-token
// classification.
//
// Group table entry (uint2), indexed by the next kLutBits stream bits:
//   .x  the first 4 output bytes of the group (0 where the output is a zero)
//   .y  [4:0]   code bits of the whole group   [9:5]   extra bits that follow them
//       [18:10] symbols it produces, before the extra-bits value is added
//       [22:19] code bits of its first token    [25:23] class of the first token:
//               0 literal / single zero, 1 two zeros, 2..5 zero runs 257..260
//       [31:27] [4:0] + [9:5]: the bits the step consumes
//       (so the extra-bits value is v_bfe_u32(window, y, y >> 5) -- the hardware
//       takes the low five bits of either operand -- and the step is five
//       instructions from the table word to the new window)
//   .y == 0: the first code is longer than the table; .x says where to continue:
//            bit 31 set: second-level table (offset << 8 | index bits), whose
//            entries are step words of ONE token (sub_leaf) or node references;
//            else node | depth << 16 for the tree walk.
// A lane owns the tokens that START in [start, lim): the whole group is taken
// while pos + kLutBits <= lim (every token of it then starts before lim), the
// first token alone otherwise.
// ---------------------------------------------------------------------------
constexpr int kWinBytes = 32768;  // output window in LDS (streams that go to HBM)
constexpr uint32_t kMinSubBits = 128;  // shortest sub-sequence a lane decodes (short rows: more lanes busy)
constexpr int kPayWords = 9216 + 8;     // k_row_count: LDS words for a row's payload
constexpr uint32_t kPayPad = 4;         // dwords past the payload the reader may touch (window look-ahead)
constexpr uint32_t kJoinBits = 64;     // a moved lane re-joins its earlier decode this far past its nominal start

struct GrpTables {
  const uint2 *grp;           // LDS: 1 << kLutBits first-level entries, then kSubEntries
                              // second-level entries (.x bytes / descriptor, .y step word)
  const uint32_t *gx, *gy;    // the same two tables as two arrays, each (1 << kLutBits) +
                              // kSubEntries long, gx right behind gy (count-only kernels:
                              // the hot read is .y alone, and a stride-2 dword read of the
                              // interleaved table uses every other LDS bank only)
  const uint32_t *nd;         // LDS tree nodes: child a | child b << 10 | (symbol + 1) << 20
};
constexpr int kTabEntries = (1 << kLutBits) + kSubEntries;

// The decode tables of one stream as they sit in LDS (interleaved form).
struct __attribute__((aligned(16))) LdsTables {
  uint2 grp[kTabEntries];
  uint32_t nd[kMaxNodes + 1];
};
__device__ __forceinline__ GrpTables tables_of(const LdsTables *T) {
  GrpTables t;
  t.grp = T->grp; t.gx = nullptr; t.gy = nullptr; t.nd = T->nd;
  return t;
}

// LDS byte address of a pointer into LDS, and loads through such an address (the
// hot loops keep "which table, how many index bits" as an address and a mask).
typedef const __attribute__((address_space(3))) uint32_t *lds_u32p;
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
__device__ __forceinline__ uint32_t lds_ld32(uint32_t a) { return *(lds_u32p)(uintptr_t)a; }
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 lds_ld64(uint32_t a) {
  const u32x2 v = *(const __attribute__((address_space(3))) u32x2 *)(uintptr_t)a;
  return make_uint2(v.x, v.y);
}

// Exclusive scan of a 64-bit value over the 1024-thread workgroup.
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v,
                                                             unsigned long long *sm,
                                                             unsigned long long *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) sm[wave] = incl;
  __syncthreads();
  unsigned long long pre = 0, tot = 0;
  for (int w = 0; w < kDecThreads / 64; ++w) {
    if (w < wave) pre += sm[w];
    tot += sm[w];
  }
  __syncthreads();
  *total = tot;
  return pre + incl - v;
}

struct StreamShared {            // small LDS state of the stream decoder
  uint32_t nxt[kDecThreads + 1];
  unsigned long long sm64[kDecThreads / 64];
  unsigned long long endbit;     // bits consumed when the output became complete
  int flag;
  int err;
  uint32_t dbg[2];               // diagnostics: lanes that re-joined / re-decoded in rounds >= 2
};

// Bit window over the stream's dwords in global memory.  Word indices are
// clamped to the dword that holds the stream's last byte: bits past the end of
// the stream repeat that dword, which only a token that overruns the payload can
// see -- and such a stream is rejected whatever those bits are.
template <class PTR>
struct ReaderT {
  PTR w;               // dword-aligned window base (global memory, or LDS for a staged payload)
  uint32_t jmax;       // index of the stream's last dword
  unsigned long long win;
  int nb;              // valid bits in win
  uint32_t next;       // index of the word held in pre
  uint32_t pre;        // prefetched word: the load issued by one refill is first
                       // touched by the next one, so its latency hides behind ~3 steps.
                       // (It must land in `pre` untouched -- any move or mask of the
                       // loaded register makes the compiler wait for it on the spot.)
  // Window over the stream `p` (4-byte aligned, stream_size bytes) whose bit 0 is
  // the dword holding absolute stream bit abs_bit; returns abs_bit's offset in it.
  __device__ __forceinline__ uint32_t attach(const uint8_t *p, uint32_t stream_size,
                                             unsigned long long abs_bit) {
    const uint32_t gb = (uint32_t)(abs_bit >> 5) * 4u;
    w = (PTR)reinterpret_cast<const uint32_t *>(p + gb);
    jmax = ((stream_size - 1u) >> 2) - (gb >> 2);
    return (uint32_t)(abs_bit - 8ull * gb);
  }
  __device__ __forceinline__ uint32_t ld(uint32_t j) const { return w[j < jmax ? j : jmax]; }
  __device__ __forceinline__ void init(uint32_t pos) {
    const uint32_t j = pos >> 5, sh = pos & 31;
    win = (((unsigned long long)ld(j + 1) << 32) | ld(j)) >> sh;
    nb = 64 - (int)sh;
    next = j + 2;
    pre = ld(next);
  }
  __device__ __forceinline__ void refill() {   // afterwards nb >= 33
    if (nb <= 32) {
      win |= (unsigned long long)pre << nb;
      nb += 32;
      ++next;
      pre = ld(next);
    }
  }
  __device__ __forceinline__ void consume(int n) { win >>= n; nb -= n; }
  // End of a walk: the last prefetch is never used, and a load that is still in flight when
  // the walk's code is left stays "pending" on its register for the compiler's s_waitcnt
  // placement in whatever code follows -- including, through the structurised control flow,
  // loops of OTHER walks that can never run after this one: their ds_read into that register
  // then carries an s_waitcnt vmcnt(0) on every iteration (round 5: the chain loop of the row
  // kernel's write pass waited for its own prefetch on every step because the token-tail
  // loop's prefetch register was still pending on a static path into it).  Using the word
  // here makes the wait happen once, where the walk ends.
  __device__ __forceinline__ void retire() { asm volatile("" :: "v"(pre)); }
};
typedef ReaderT<const uint32_t *> GReader;                                        // payload in place (L2)
typedef ReaderT<const __attribute__((address_space(3))) uint32_t *> LReader;      // payload staged in LDS

// Words [0, n) of a global reader's window -> LDS (dst 16-byte aligned, room for n
// rounded up to 4): four words per lane and step with ONE 16-byte load (the stream is
// only dword aligned; global memory takes that), so a 33 KiB row is three loads per
// lane in flight instead of nine one after the other.  Words past the stream's last
// dword repeat it, exactly like ReaderT::ld, and nothing past it is read.
struct __attribute__((packed, aligned(4))) PackedU4 { uint32_t x, y, z, w; };
__device__ __forceinline__ void stage_payload(const GReader &rd, uint32_t *dst, uint32_t n) {
  for (uint32_t k = threadIdx.x; 4u * k < n; k += kDecThreads) {
    uint4 v;
    if (4u * k + 3u <= rd.jmax) {
      const PackedU4 q = *reinterpret_cast<const PackedU4 *>(rd.w + 4u * k);
      v.x = q.x; v.y = q.y; v.z = q.z; v.w = q.w;
    } else {
      v.x = rd.ld(4u * k); v.y = rd.ld(4u * k + 1u); v.z = rd.ld(4u * k + 2u); v.w = rd.ld(4u * k + 3u);
    }
    *reinterpret_cast<uint4 *>(dst + 4u * k) = v;
  }
}

// Extra bits and run base per token class (huffman_common.h:24-28).
__device__ __forceinline__ uint32_t class_eb(uint32_t c) { return (0xE84200u >> (4u * c)) & 15u; }
__device__ __forceinline__ uint32_t class_base(uint32_t c) {
  const unsigned long long kBases = 1ull | (2ull << 9) | (3ull << 18) | (7ull << 27) | (23ull << 36) | (279ull << 45);
  return (uint32_t)(kBases >> (9u * c)) & 511u;
}

// The step word of a group entry reduced to its FIRST token (a lane's last
// kLutBits bits: it owns the tokens that START in its range).
__device__ __forceinline__ uint32_t first_token_word(uint32_t y) {
  const uint32_t c = (y >> 23) & 7u, tb = (y >> 19) & 15u, eb = class_eb(c);
  return tb | (eb << 5) | (class_base(c) << 10) | ((tb + eb) << 27);
}

// The tree walk for whatever neither table resolves (huffman_dec.cpp:291-328): from
// the node and depth in x (node | depth << 16; 0: nothing there), `base` code bits of
// the token already consumed from the window.  Consumes the rest of the code, returns
// a step word whose code-bit count is 0 (only the extra bits are left to take);
// *len_out = the code's length, *byte = the literal (0 for runs).  bad is set (never
// cleared) on symbols the reference rejects (huffman_dec.cpp:349-352).
template <class RD>
__device__ __forceinline__ uint32_t walk_token(RD &rd, const GrpTables &t, uint32_t x, int base,
                                               uint32_t *len_out, uint32_t *byte, bool *bad) {
  int node = (int)(x & 0xffffu), len = (int)((x >> 16) & 0x7fffu);
  uint32_t nd = t.nd[node];
  while (len >= base && (nd >> 20) == 0 && len < kMaxDepth) {
    node = (int)(((rd.win >> (len - base)) & 1ull) ? (nd >> 10) & 1023u : nd & 1023u);
    nd = t.nd[node];
    ++len;
  }
  const int sym = (int)(nd >> 20) - 1;
  const bool ok = sym >= 0 && sym <= 260 && len > base;
  if (!ok) *bad = true;
  if (len <= base) len = base + 1;  // keep moving on a degenerate tree
  rd.consume(len - base);
  rd.refill();
  *len_out = (uint32_t)len;
  const uint32_t c = !ok ? 0u : (sym < 256 ? 0u : (uint32_t)sym - 255u);
  const uint32_t eb = class_eb(c);
  *byte = (ok && sym < 256) ? (uint32_t)sym : 0u;
  return (eb << 5) | ((ok ? class_base(c) : 0u) << 10) | (eb << 27);
}

// A token whose code is longer than the first-level table, resolved in ONE call (the
// tails and the exact paths; the hot loops spread it over two steps instead, see
// lean_count): second-level table, the tree below it for whatever is deeper still.
// Consumes the code bits and returns a step word whose code-bit count is 0.
// *pre = code bits consumed, *byte = the literal (0 for runs).
template <bool SOA, class RD>
__device__ __forceinline__ uint32_t long_token(RD &rd, const GrpTables &t, uint32_t idx, uint32_t *pre,
                                            uint32_t *byte, bool *bad) {
  uint32_t x = SOA ? t.gx[idx] : t.grp[idx].x;
  int base = 0;
  if (x >> 31) {
    rd.consume(kLutBits);
    rd.refill();
    base = kLutBits;
    const uint32_t j = (1u << kLutBits) + ((x >> 8) & 0xffffu) + __builtin_amdgcn_ubfe((uint32_t)rd.win, 0, x & 255u);
    const uint32_t y2 = SOA ? t.gy[j] : t.grp[j].y;
    x = SOA ? t.gx[j] : t.grp[j].x;
    if (y2) {   // resolved: the common case by far
      const uint32_t rest = y2 & 31u, eb = (y2 >> 5) & 31u;
      rd.consume((int)rest);
      rd.refill();
      *pre = kLutBits + rest;
      *byte = x;
      return (y2 & 0x0007ffe0u) | (eb << 27);
    }
  }
  return walk_token(rd, t, x, base, pre, byte, bad);
}

// One decode step in its general form (the tails and the exact paths; the hot
// loops below inline the same thing without the `single` test).
template <bool WANT_BYTES, bool SOA = false, class RD = GReader>
__device__ __forceinline__ void lean_step(RD &rd, const GrpTables &t, bool single,
                                          uint32_t *nbits, uint32_t *count, uint32_t *bytes,
                                          bool *bad) {
  rd.refill();
  const uint32_t idx = (uint32_t)rd.win & ((1u << kLutBits) - 1u);
  uint32_t y, by = 0, pre = 0;
  if (WANT_BYTES) { const uint2 e = t.grp[idx]; by = e.x; y = e.y; }
  else if (SOA) y = t.gy[idx];
  else y = reinterpret_cast<const uint32_t *>(t.grp)[2 * idx + 1];
  if (__builtin_expect(y == 0, 0)) {
    y = long_token<SOA>(rd, t, idx, &pre, &by, bad);
  } else if (single) {
    y = first_token_word(y);
    by &= 255u;
  }
  const uint32_t extra = __builtin_amdgcn_ubfe((uint32_t)rd.win, y, y >> 5);   // the hardware takes [4:0] of either
  const uint32_t n = y >> 27;
  rd.consume((int)n);
  *nbits = pre + n;
  *count = ((y >> 10) & 511u) + extra;
  *bytes = by;
}

// Count pass: the tokens that start in [pos, lim).  Returns where the last one
// ends and how many symbols they produce.  Two loops: whole groups while every
// token of a group is sure to start before lim (pos + kLutBits <= lim), single
// tokens for the last few bits -- so that the hot loop carries no `single` test.
// cont: the reader already stands at pos (a previous call ended there).
// GRP: the lane owns the GROUPS that start in [pos, lim) -- one loop, no single-token
// tail; the walk ends at the first group boundary at or past lim (up to kLutBits + 14
// bits behind it).  Any token boundary divides two lanes' ranges correctly as long as
// the consumer walks from its own start to its right neighbour's start (the row kernels
// do), so the count kernels need not agree on a canonical one.
template <bool SOA = false, class RD = GReader, bool GRP = false>
__device__ __forceinline__ void lean_count(RD &rd, const GrpTables &t, uint32_t pos,
                                           uint32_t lim, uint32_t *endpos, uint32_t *count,
                                           bool cont = false) {
  uint32_t c = 0;
  if (pos < lim) {
    if (!cont) rd.init(pos);
    const int limk = (int)lim - kLutBits;
    bool bad = false;
    // The table a step indexes is lane state (tm: index mask, tb: LDS address, both in
    // bytes): a code longer than the first-level table is NOT resolved on the spot --
    // that was a 40-instruction detour with two dependent LDS reads which the whole
    // wavefront waited for whenever one of its 64 lanes met such a code (57 % of the
    // steps) -- but taken as a step that consumes the kLutBits known bits, produces
    // nothing and points the lane's NEXT step at the code's second-level table.
    constexpr int SH = SOA ? 2 : 3;
    const uint32_t TM = ((1u << kLutBits) - 1u) << SH;
    const uint32_t TB = SOA ? lds_addr(t.gy) : lds_addr(t.grp) + 4u;   // the .y words
    const uint32_t XOFF = SOA ? (uint32_t)kTabEntries * 4u : 0xfffffffcu;   // from .y to its .x
    uint32_t tm = TM, tb = TB;
    auto step = [&]() {
      rd.refill();
      const uint32_t a = ((((uint32_t)rd.win) << SH) & tm) + tb;
      uint32_t y = lds_ld32(a);
      uint32_t ntm = TM, ntb = TB, adv = 0;
      if (__builtin_expect(y == 0, 0)) {
        const uint32_t x = lds_ld32(a + XOFF);
        if ((x >> 31) && tm == TM) {
          ntm = ((1u << (x & 255u)) - 1u) << SH;
          ntb = TB + (((1u << kLutBits) + ((x >> 8) & 0xffffu)) << SH);
          y = (uint32_t)kLutBits | ((uint32_t)kLutBits << 27);
        } else {
          const int base = tm == TM ? 0 : kLutBits;
          uint32_t len, by;
          y = walk_token(rd, t, x, base, &len, &by, &bad);
          adv = len - (uint32_t)base;
        }
      }
      tm = ntm; tb = ntb;
      const uint32_t extra = __builtin_amdgcn_ubfe((uint32_t)rd.win, y, y >> 5);
      const uint32_t n = y >> 27;
      rd.consume((int)n);
      pos += adv + n;
      c += ((y >> 10) & 511u) + extra;
    };
    if constexpr (GRP) {
      while (pos < lim) step();
      if (tm != TM) step();
    } else {
      while ((int)pos <= limk) step();
      if (tm != TM) step();   // the loop ended between the two steps of a long code
      while (pos < lim) {
        uint32_t nbits, cnt, by;
        lean_step<false, SOA>(rd, t, true, &nbits, &cnt, &by, &bad);
        pos += nbits;
        c += cnt;
      }
    }
  }
  rd.retire();
  *endpos = pos;
  *count = c;
}

// Speculative decode of one chunk to the self-synchronised fixpoint.  On return
// lane t owns exactly the tokens that START in [*start, lim) -- given that lane
// 0's start `first` is exact (asserted or assumed by the caller).
// Cold: *start = nominal start, the lane decodes in round 1 iff `active`.
// Warm: (*start, *endpos, *cnt) hold a fixpoint reached for another `first`; only
// lanes whose start changes decode again.
// Lanes whose range lies beyond the payload (`active` false) own nothing and stay
// out of it: passing the chain's end along them would cost one round per lane.
// MEMO > 0: the lane remembers its last MEMO (start -> end, count) results in
// memo[3 * MEMO] (start ~0u = empty; the caller may pre-load it) and a start it has
// seen before costs a look-up.  For streams that do NOT self-synchronise -- codes of
// nearly one length, e.g. the 5/6-bit codes of the LRES predictor bytes: a wrong
// phase survives thousands of tokens there -- every round moves every lane of such a
// stretch to one of the same few phases again, and the correction passes along the
// chain one lane per round: rounds that are look-ups instead of decodes.
// NQ > 0: the lane's walk is cut at NQ more marks (mark[k], non-decreasing, between the
// re-join point and lim): on return mark[k] = the first token boundary at or past the mark
// and mcnt[k] = the symbols of the lane's tokens in front of it (k_row_count for rows that
// go through windows: four records per lane).
template <bool SOA = false, class RD = GReader, int MEMO = 0, int NQ = 0>
__device__ __forceinline__ void lean_fixpoint(RD &rd, const GrpTables &tb, StreamShared *sh,
                                              uint32_t first, bool active, uint32_t lim,
                                              uint32_t *start_io, uint32_t *endpos_io,
                                              uint32_t *cnt_io, uint32_t *rounds, bool warm,
                                              uint32_t lead_bits, long long *c_first = nullptr,
                                              long long *c_phase = nullptr, uint32_t *memo = nullptr,
                                              uint32_t *mark = nullptr, uint32_t *mcnt = nullptr) {
  const int tid = threadIdx.x;
  const long long t_in = clock64();
  uint32_t start = *start_io, endpos = *endpos_io, cnt = *cnt_io;
  const uint32_t nominal = start;   // cold: the lane's nominal boundary
  bool dirty = active;
  if (tid == 0 && !warm) start = first;
  // Lead-in: instead of starting blind at its nominal boundary, a lane decodes the
  // last lead_bits of its left neighbour's range first.  Huffman codes resynchronise
  // within a few tokens, so the first token boundary at or past the nominal start
  // found that way is almost always the true one, and round 1 is then already the
  // final round (1 + lead_bits/sub passes over the payload instead of 2+).  A lane
  // that did not synchronise is corrected by the rounds below as before.
  if (!warm && tid > 0 && active && lead_bits) {
    const uint32_t from = start - first > lead_bits ? start - lead_bits : first;
    uint32_t guess, none;
    lean_count<SOA>(rd, tb, from, start, &guess, &none);
    start = guess;
  }
  if (c_phase) c_phase[0] = clock64() - t_in;   // lead-in (this wave)
  if (warm) {
    dirty = (tid == 0) && (first != start);
    if (dirty) start = first;
  }
  // Re-join: a lane's decode is cut at T = nominal start + kJoinBits.  It remembers
  // the first token boundary at or past T (canonical: whatever the grouping, the
  // group that crosses T ends with a token that started before T) and the symbols
  // up to it.  When its start moves in a later round it decodes up to T again; if it
  // arrives at the same boundary, everything behind is what it already has -- the
  // end stays, the count is adjusted -- and the round costs kJoinBits instead of the
  // whole sub-sequence (codes resynchronise within a few tokens, so almost every
  // moved lane re-joins).
  uint32_t T = nominal + kJoinBits;
  if (T > lim || T < nominal) T = lim;
  uint32_t posT = ~0u, cT = 0;
  uint32_t mk[NQ > 0 ? NQ : 1], mp[NQ > 0 ? NQ : 1], mc[NQ > 0 ? NQ : 1];
  if (NQ > 0) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      uint32_t m = mark[k];
      if (m < T) m = T;
      if (m > lim) m = lim;
      mk[k] = m; mp[k] = start; mc[k] = 0;
    }
  }
  for (;;) {
    bool hit = false;
    if (MEMO > 0 && dirty) {
#pragma unroll
      for (int e = 0; e < MEMO; ++e)
        if (memo[3 * e] == start) { endpos = memo[3 * e + 1]; cnt = memo[3 * e + 2]; hit = true; }
      if (hit) posT = ~0u;   // (endpos, cnt) no longer belong to the re-join checkpoint
    }
    if (dirty && !hit) {
      uint32_t p1, c1;
      lean_count<SOA>(rd, tb, start, T, &p1, &c1);
      if (p1 == posT) {
        cnt = c1 + (cnt - cT);
        if (NQ > 0) {
#pragma unroll
          for (int k = 0; k < NQ; ++k) mc[k] += c1 - cT;
        }
        if (*rounds) atomicAdd(&sh->dbg[0], 1u);
      } else {
        if (*rounds) atomicAdd(&sh->dbg[1], 1u);
        uint32_t c2, pos = p1, acc = c1;
        bool at = start < T;   // the reader stands at `pos`
        if (NQ > 0) {
#pragma unroll
          for (int k = 0; k < NQ; ++k) {
            uint32_t ck;
            lean_count<SOA>(rd, tb, pos, mk[k], &mp[k], &ck, at);
            at = at || pos < mk[k];
            pos = mp[k];
            acc += ck;
            mc[k] = acc;
          }
        }
        lean_count<SOA>(rd, tb, pos, lim, &endpos, &c2, at);
        cnt = acc + c2;
      }
      posT = p1;
      cT = c1;
      if (MEMO > 0) {
#pragma unroll
        for (int e = MEMO - 1; e > 0; --e) {
          memo[3 * e] = memo[3 * e - 3]; memo[3 * e + 1] = memo[3 * e - 2]; memo[3 * e + 2] = memo[3 * e - 1];
        }
        memo[0] = start; memo[1] = endpos; memo[2] = cnt;
      }
    }
    sh->nxt[tid + 1] = endpos;
    __syncthreads();
    if (c_first && *c_first == 0) *c_first = clock64() - t_in;
    if (c_phase && c_phase[1] == 0) c_phase[1] = clock64() - t_in;   // end of round 1 (after its barrier)
    const uint32_t ns = tid == 0 ? first : sh->nxt[tid];
    dirty = active && (ns != start);
    if (active) start = ns;
    ++*rounds;
    if (!__syncthreads_or(dirty ? 1 : 0)) break;
  }
  *start_io = start;
  *endpos_io = endpos;
  *cnt_io = cnt;
  if (NQ > 0) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) { mark[k] = active ? mp[k] : start; mcnt[k] = active ? mc[k] : 0u; }
  }
}

// Write pass of one lane straight into LDS: the tokens that start in [bp, lim)
// go to lds_out (pre-zeroed) from offset op.  The group's bytes are OR-ed in with
// two aligned ds_or (the bytes past the group are zeros, so neighbours are never
// disturbed).  The caller guarantees that all of the lane's symbols lie strictly
// inside the block.  Same two loops as lean_count.
// CLIP: lds_out is a WINDOW of the block (k_row_window): op counts from kWinGuard
// bytes in front of the window's first symbol and the lane's symbols may lie before,
// inside or behind it; a group is OR-ed in when its first byte is less than 8 bytes in
// front of the window or inside it (win_span = window bytes + kWinGuard: one unsigned
// compare), so the two dwords it touches stay inside [0, win_span + 8).
constexpr uint32_t kWinGuard = 16;
constexpr uint32_t kRowWindow = 128u * 1024u;   // k_row_window: symbols of a row per workgroup (64 KiB windows, two
                                                // workgroups per CU: 1.12 -> 1.69 ms at 16384^2 -- half the lanes idle,
                                                // the per-workgroup costs twice)
// The chain form of lean_write (the reader stands at bp): [bp, lim) is a stretch of
// k_row_count_w's chain of groups, the groups taken from bp end exactly at lim.  The loop is bound
// by its VALU instructions (four wavefronts per SIMD; an instruction more per step is 1 % of the
// row kernel), scalar ones are free beside them.  Against lean_write's step:
//  * the verdict is a lane VALUE that only the tree walk touches (as a bool it lived in scalar
//    mask registers, three scalar instructions per step for a flag no valid stream sets);
//  * the reader's window base is the wavefront's (a row's payload): scalar base + a lane BYTE
//    offset -- the refill's address is one add and one min, the load takes the offset as it is;
//  * the output position carries the LDS address of the symbol area: the group's dword address is
//    one AND;
//  * a tree walk's extra bits advance the position where they are found, not through a register
//    that is zero on every other step.
struct ChainReader {
  unsigned long long win;
  int nb;
  uint32_t pre, noff, offmax;   // the prefetched word, its byte offset, the offset of the stream's last dword
  const __attribute__((address_space(1))) uint8_t *sbase;   // (wavefront-uniform; global)
  __device__ __forceinline__ void refill() {   // afterwards nb >= 33
    if (nb <= 32) {
      win |= (unsigned long long)pre << nb;
      nb += 32;
      noff += 4u;
      pre = *(const __attribute__((address_space(1))) uint32_t *)(sbase + min(noff, offmax));
    }
  }
  __device__ __forceinline__ void consume(int n) { win >>= n; nb -= n; }
};
__device__ __forceinline__ void lds_or32(uint32_t a, uint32_t v) {
  (void)__hip_atomic_fetch_or((__attribute__((address_space(3))) uint32_t *)(uintptr_t)a, v, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_WORKGROUP);
}
// CLIP (k_row_window): as in lean_write -- lds_out is a window of the block, a group is OR-ed in when its first byte
// lies less than 8 bytes in front of the window or inside it.
template <bool CLIP = false>
__device__ __forceinline__ bool lean_write_chain(GReader &rd0, const GrpTables &t, uint32_t bp, uint32_t lim, uint32_t op,
                                                 uint8_t *lds_out, uint32_t win_span = 0) {
  ChainReader rd;
  rd.win = rd0.win; rd.nb = rd0.nb; rd.pre = rd0.pre;
  rd.noff = 4u * rd0.next; rd.offmax = 4u * rd0.jmax;
  {
    const unsigned long long a = (unsigned long long)(uintptr_t)rd0.w;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    rd.sbase = (const __attribute__((address_space(1))) uint8_t *)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  }
  uint32_t badv = 0;
  uint32_t opa = op + lds_addr(lds_out);   // (the symbol area is dword aligned: opa & 3 == op & 3)
  const uint32_t clip_lo = lds_addr(lds_out) + (kWinGuard - 8u), clip_span = win_span - (kWinGuard - 8u);   // (CLIP)
  // (the table a step indexes is lane state: index bits and base -- v_bfe, v_lshl_add)
  const uint32_t TW = (uint32_t)kLutBits, TB = lds_addr(t.grp);
  uint32_t tm = TW, tb = TB;
  auto step = [&]() {
    rd.refill();
    const uint2 e = lds_ld64((__builtin_amdgcn_ubfe((uint32_t)rd.win, 0u, tm) << 3) + tb);
    uint32_t y = e.y, by = e.x, ntm = TW, ntb = TB;
    if (__builtin_expect(y == 0, 0)) {
      if ((by >> 31) && tm == TW) {
        ntm = by & 255u;
        ntb = TB + (((1u << kLutBits) + ((by >> 8) & 0xffffu)) << 3);
        y = (uint32_t)kLutBits | ((uint32_t)kLutBits << 27);
        by = 0;
      } else {
        const int base = tm == TW ? 0 : kLutBits;
        uint32_t len;
        bool b = false;
        y = walk_token(rd, t, by, base, &len, &by, &b);
        badv |= b ? 1u : 0u;
        bp += len - (uint32_t)base;
      }
    }
    tm = ntm; tb = ntb;
    const uint32_t extra = __builtin_amdgcn_ubfe((uint32_t)rd.win, y, y >> 5);
    const uint32_t n = y >> 27;
    rd.consume((int)n);
    if (!CLIP || opa - clip_lo < clip_span) {
      const unsigned long long v = (unsigned long long)by << (8u * (opa & 3u));
      const uint32_t a = opa & ~3u;
      lds_or32(a, (uint32_t)v);
      lds_or32(a + 4u, (uint32_t)(v >> 32));
    }
    opa += ((y >> 10) & 511u) + extra;
    bp += n;
  };
  LoopCount lc;
  while (bp < lim) { HIMG_REGION_BEGIN("dec.write"); step(); lc.step(); HIMG_REGION_END("dec.write"); }
  lc.done(0);
  if (tm != TW) step();
  asm volatile("" :: "v"(rd.pre));   // (ReaderT::retire)
  return badv == 0;
}

// chain: [bp, lim) is a stretch of k_row_count_w's chain of groups (lane_off's valid flag
// 3): the groups taken from bp end exactly at lim, one loop without a token-by-token tail.
template <bool CLIP = false>
__device__ __forceinline__ bool lean_write(GReader &rd, const GrpTables &t, uint32_t bp,
                                           uint32_t lim, uint32_t op, uint8_t *lds_out, uint32_t win_span = 0,
                                           bool chain = false) {
  bool bad = false;
  if (bp < lim) {
    rd.init(bp);
    const int limk = (int)lim - kLutBits;
    uint32_t *o32 = reinterpret_cast<uint32_t *>(lds_out);
    // Long codes: two steps, the table being lane state (see lean_count).
    const uint32_t TM = ((1u << kLutBits) - 1u) << 3, TB = lds_addr(t.grp);
    uint32_t tm = TM, tb = TB;
    auto step = [&]() {
      rd.refill();
      const uint2 e = lds_ld64(((((uint32_t)rd.win) << 3) & tm) + tb);
      uint32_t y = e.y, by = e.x, ntm = TM, ntb = TB, adv = 0;
      // (Unconditional: resetting the table state only on the rare paths -- an else-branch on
      // tm != TM -- trades three v_mov for four scalar instructions and a branch per step and
      // measured 12 % slower in the count kernel, 2 % in the row kernel.)
      if (__builtin_expect(y == 0, 0)) {
        if ((by >> 31) && tm == TM) {
          ntm = ((1u << (by & 255u)) - 1u) << 3;
          ntb = TB + (((1u << kLutBits) + ((by >> 8) & 0xffffu)) << 3);
          y = (uint32_t)kLutBits | ((uint32_t)kLutBits << 27);
          by = 0;
        } else {
          const int base = tm == TM ? 0 : kLutBits;
          uint32_t len;
          y = walk_token(rd, t, by, base, &len, &by, &bad);
          adv = len - (uint32_t)base;
        }
      }
      tm = ntm; tb = ntb;
      const uint32_t extra = __builtin_amdgcn_ubfe((uint32_t)rd.win, y, y >> 5);
      const uint32_t n = y >> 27;
      rd.consume((int)n);
      if (!CLIP || op - (kWinGuard - 8u) < win_span - (kWinGuard - 8u)) {
        const unsigned long long v = (unsigned long long)by << (8u * (op & 3u));
        atomicOr(&o32[op >> 2], (uint32_t)v);
        atomicOr(&o32[(op >> 2) + 1], (uint32_t)(v >> 32));
      }
      op += ((y >> 10) & 511u) + extra;
      bp += adv + n;
    };
    if (chain) return lean_write_chain<CLIP>(rd, t, bp, lim, op, lds_out, win_span);   // (uniform per row)
    while ((int)bp <= limk) step();
    if (tm != TM) step();
    while (bp < lim) {
      uint32_t nbits, cnt, by;
      lean_step<true>(rd, t, true, &nbits, &cnt, &by, &bad);
      if (by && (!CLIP || op - kWinGuard < win_span - kWinGuard)) lds_out[op] = (uint8_t)by;
      op += cnt;
      bp += nbits;
    }
    rd.retire();
  }
  return !bad;
}

// The lane in whose range the block completes: exact token-by-token decode with
// the reference's end-of-block checks (huffman_dec.cpp:353-354,361-417).
// Returns false on a stream error; *end_bp = bit position where the block became
// complete (~0u if it did not).
// CLIP: as in lean_write; op and out_size then both count from the window's guard.
template <bool CLIP = false>
__device__ __forceinline__ bool exact_write_body(GReader &rd, const GrpTables &t, uint32_t bp,
                                                 uint32_t lim, uint32_t op, uint32_t out_size,
                                                 uint8_t *lds_out, uint32_t *end_bp, uint32_t win_span) {
  *end_bp = ~0u;
  // Positions are compared as SIGNED numbers: in a window (CLIP) a lane may start in
  // front of it, its position then lies below zero (everything is far below 2^31).
  const auto before = [](uint32_t a, uint32_t b) { return (int32_t)a < (int32_t)b; };
  if (!(bp < lim) || !before(op, out_size)) return true;
  rd.init(bp);
  bool bad = false;
  // Whole groups first, as long as the block stays incomplete behind them: this lane is
  // alone on its path while fifteen wavefronts wait at the barrier behind the write
  // pass -- token by token over its whole range (~50 tokens, each a dependent LDS
  // round trip) it was HALF of that pass.  The group that completes (or overruns) the
  // block is not taken: the reader is put back in front of it and the loop below goes
  // through it token by token with the reference's checks.
  {
    const int limk = (int)lim - kLutBits;
    uint32_t *o32 = reinterpret_cast<uint32_t *>(lds_out);
    while ((int)bp <= limk) {
      const GReader saved = rd;
      uint32_t nbits, cnt, by;
      bool gbad = false;
      lean_step<true>(rd, t, false, &nbits, &cnt, &by, &gbad);
      if (gbad || !before(op + cnt, out_size)) { rd = saved; break; }
      if (!CLIP || op - (kWinGuard - 8u) < win_span - (kWinGuard - 8u)) {
        const unsigned long long v = (unsigned long long)by << (8u * (op & 3u));
        atomicOr(&o32[op >> 2], (uint32_t)v);
        atomicOr(&o32[(op >> 2) + 1], (uint32_t)(v >> 32));
      }
      op += cnt;
      bp += nbits;
    }
  }
  for (;;) {
    uint32_t nbits, cnt, by;
    lean_step<true>(rd, t, true, &nbits, &cnt, &by, &bad);
    if (bad) return false;
    if (before(out_size, op + cnt)) return false;  // a zero run overruns the block
    if (by && (!CLIP || op - kWinGuard < win_span - kWinGuard)) lds_out[op] = (uint8_t)by;
    op += cnt;
    bp += nbits;
    if (!before(op, out_size)) { *end_bp = bp; return true; }
    if (!(bp < lim)) return true;
  }
}

template <bool CLIP = false>
__device__ __forceinline__ bool exact_write(GReader &rd, const GrpTables &t, uint32_t bp,
                                            uint32_t lim, uint32_t op, uint32_t out_size,
                                            uint8_t *lds_out, uint32_t *end_bp, uint32_t win_span = 0) {
  const bool ok = exact_write_body<CLIP>(rd, t, bp, lim, op, out_size, lds_out, end_bp, win_span);
  rd.retire();   // (whichever way the walk ended: see ReaderT::retire)
  return ok;
}

// Write pass to HBM through 32 KiB LDS windows (zero runs are the window's zero
// fill; windows are flushed with 16-byte stores).  Lane t decodes the tokens that
// start in [bp, lim) and places them from output offset op; `exact` marks the lane
// in whose range the block completes.  win holds kWinBytes / 4 + 1 words.
__device__ __forceinline__ void lean_write_windows(GReader &rd, const GrpTables &tb,
                                                   StreamShared *sh, uint32_t bp, uint32_t lim,
                                                   unsigned long long op, bool exact,
                                                   unsigned long long O0, unsigned long long O1,
                                                   uint32_t out_size,
                                                   unsigned long long endbit_base, uint32_t rel0,
                                                   uint32_t *win, uint8_t *gout) {
  const int tid = threadIdx.x;
  bool done = !(bp < lim) || op >= out_size;
  bool bad = false;
  if (!done) rd.init(bp);
  const int limk = (int)lim - kLutBits;
  for (unsigned long long wb = (O0 / kWinBytes) * kWinBytes; wb < O1; wb += kWinBytes) {
    for (int k = tid; k < kWinBytes / 4 + 1; k += kDecThreads) win[k] = 0;
    __syncthreads();
    const unsigned long long we = wb + kWinBytes;
    while (!done && op < we) {
      // The explicit bytes of a group may not straddle the window end.
      const bool single = exact || (int)bp > limk || op + 4 > we;
      uint32_t nbits, cnt, by;
      lean_step<true>(rd, tb, single, &nbits, &cnt, &by, &bad);
      if (exact && (bad || op + cnt > out_size)) { bad = true; break; }
      const uint32_t o = (uint32_t)(op - wb);
      const unsigned long long v = (unsigned long long)by << (8u * (o & 3u));
      atomicOr(&win[o >> 2], (uint32_t)v);
      atomicOr(&win[(o >> 2) + 1], (uint32_t)(v >> 32));
      op += cnt;
      bp += nbits;
      if (exact && op >= out_size) { sh->endbit = endbit_base + (bp - rel0); done = true; }
      else if (!(bp < lim)) done = true;
    }
    if (bad) { sh->err = 1; done = true; }
    __syncthreads();
    // Flush [max(wb, O0), min(we, O1)): 16-byte stores inside, bytes at the edges
    // (another workgroup may own the rest of an edge group).
    const unsigned long long lo = wb > O0 ? wb : O0, hi = we < O1 ? we : O1;
    const uint32_t l = (uint32_t)(lo - wb), h = (uint32_t)(hi - wb);
    const uint32_t la = (l + 15u) & ~15u, ha = h & ~15u;
    const uint8_t *w8 = reinterpret_cast<const uint8_t *>(win);
    if (la <= ha && (((uintptr_t)(gout + wb)) & 15) == 0) {
      for (uint32_t k = l + tid; k < la; k += kDecThreads) gout[wb + k] = w8[k];
      for (uint32_t k = la / 16 + tid; k < ha / 16; k += kDecThreads) {
        uint4 q;
        q.x = win[4 * k]; q.y = win[4 * k + 1]; q.z = win[4 * k + 2]; q.w = win[4 * k + 3];
        *reinterpret_cast<uint4 *>(gout + wb + 16ull * k) = q;
      }
      for (uint32_t k = ha + tid; k < h; k += kDecThreads) gout[wb + k] = w8[k];
    } else {
      for (uint32_t k = l + tid; k < h; k += kDecThreads) gout[wb + k] = w8[k];
    }
    __syncthreads();
  }
  rd.retire();
}

// Write pass straight to PRE-ZEROED global memory (the LRES symbols: 1/64 of the
// frame, L2 resident): lane t decodes the tokens that start in [bp, lim) and stores
// the non-zero literal bytes of every group at their final positions from op; zero
// runs and literal zeros need no store.  No LDS window, no barrier: the kernel that
// calls this keeps only the decode tables in LDS and lasts as long as one lane's 256
// bits.  `exact` marks the lane in whose range the block completes (token by token
// there, with the reference's end-of-block checks, huffman_dec.cpp:353-354,361-417).
__device__ __forceinline__ void lean_write_global(GReader &rd, const GrpTables &tb, StreamShared *sh,
                                                  uint32_t bp, uint32_t lim, unsigned long long op,
                                                  bool exact, uint32_t out_size,
                                                  unsigned long long endbit_base, uint32_t rel0,
                                                  uint8_t *gout, unsigned long long op_end) {
  if (!(bp < lim) || op >= out_size) return;
  rd.init(bp);
  const int limk = (int)lim - kLutBits;
  bool bad = false;
  if (!exact) {
    // Every lane but the one in which the block completes: lean_write's loop (whole groups,
    // a long code as two steps whose table is lane state) with the store below instead of
    // the OR into LDS; the general step further down costs twice the instructions and was
    // k_lres_write's whole time (0.74 -> 0.55 ms per 128 frames, in front of the row kernel).
    const uint32_t TM = ((1u << kLutBits) - 1u) << 3, TB = lds_addr(tb.grp);
    uint32_t tm = TM, tbase = TB;
    uint32_t o = (uint32_t)op;                       // (the output of one stream is below 2^32 symbols)
    const uint32_t o_end = (uint32_t)op_end;
    auto put = [&](uint32_t by) {
      if (by) {
        if (o + 4u <= o_end) {
          asm volatile("global_store_dword %0, %1, %2" :: "v"(o), "v"(by), "s"(gout) : "memory");
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t b = (by >> (8 * j)) & 255u;
            if (b) gout[o + j] = (uint8_t)b;
          }
        }
      }
    };
    auto step = [&]() {
      rd.refill();
      const uint2 e = lds_ld64(((((uint32_t)rd.win) << 3) & tm) + tbase);
      uint32_t y = e.y, by = e.x, ntm = TM, ntb = TB, adv = 0;
      if (__builtin_expect(y == 0, 0)) {
        if ((by >> 31) && tm == TM) {
          ntm = ((1u << (by & 255u)) - 1u) << 3;
          ntb = TB + (((1u << kLutBits) + ((by >> 8) & 0xffffu)) << 3);
          y = (uint32_t)kLutBits | ((uint32_t)kLutBits << 27);
          by = 0;
        } else {
          const int base = tm == TM ? 0 : kLutBits;
          uint32_t len;
          y = walk_token(rd, tb, by, base, &len, &by, &bad);
          adv = len - (uint32_t)base;
        }
      }
      tm = ntm; tbase = ntb;
      const uint32_t extra = __builtin_amdgcn_ubfe((uint32_t)rd.win, y, y >> 5);
      const uint32_t n = y >> 27;
      rd.consume((int)n);
      put(by);
      o += ((y >> 10) & 511u) + extra;
      bp += adv + n;
    };
    while ((int)bp <= limk) step();
    if (tm != TM) step();
    while (bp < lim) {
      uint32_t nbits, cnt, by;
      lean_step<true>(rd, tb, true, &nbits, &cnt, &by, &bad);
      put(by);
      o += cnt;
      bp += nbits;
    }
    rd.retire();
    if (bad) sh->err = 1;
    return;
  }
  for (;;) {
    uint32_t nbits, cnt, by;
    lean_step<true>(rd, tb, exact || (int)bp > limk, &nbits, &cnt, &by, &bad);
    if (exact && (bad || op + cnt > out_size)) { bad = true; break; }
    // A group's (at most 4) explicit bytes lie inside [op, op + cnt); the bytes of the
    // dword beyond them are zeros of its run or belong to this lane's NEXT groups,
    // which are stored later and in order -- so while the dword stays inside the
    // lane's own output range [.., op_end) it goes out as one (unaligned) dword store,
    // and not at all when it is zero.  Near the end of the range: byte by byte.
    if (by) {
      if (op + 4 <= op_end) {
        asm volatile("global_store_dword %0, %1, %2" :: "v"((uint32_t)op), "v"(by), "s"(gout) : "memory");
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t b = (by >> (8 * j)) & 255u;
          if (b) gout[op + j] = (uint8_t)b;
        }
      }
    }
    op += cnt;
    bp += nbits;
    if (exact && op >= out_size) { sh->endbit = endbit_base + (bp - rel0); break; }
    if (!(bp < lim)) break;
  }
  rd.retire();
  if (bad) sh->err = 1;
}

// The kDecThreads sub-sequences of one chunk of `bits` payload bits (`sb` bits each,
// bits <= kDecThreads * sb).  The boundaries lie at k * sb - S: the whole grid is moved
// to the left so that the LAST active lane is left with kTailBits -- that lane ends up
// alone on the token-by-token path that completes the block (exact_write) while every
// other wavefront of the row waits for it, so its range is kept as short as the grid
// allows (lane 0 takes what is cut off; no shift when that would need a 1025th lane).
// Every kernel that walks a chunk derives the same grid from (bits, sb).
constexpr uint32_t kTailBits = 48;
struct SubGrid {
  uint32_t b0, lim;     // this lane's range [b0, lim), window bit positions
  bool active;
  int last_active;
};
__device__ __forceinline__ SubGrid sub_grid(uint32_t rel0, uint32_t bits, uint32_t sb, int tid) {
  SubGrid q;
  const uint32_t la = (bits - 1u) / sb, L = bits - la * sb;
  const uint32_t S = (L > kTailBits && la + 1u < (uint32_t)kDecThreads) ? sb - (L - kTailBits) : 0u;
  const uint32_t rel_end = rel0 + bits;
  q.b0 = tid ? rel0 + (uint32_t)tid * sb - S : rel0;
  q.lim = rel0 + (uint32_t)(tid + 1) * sb - S;
  if (q.lim > rel_end) q.lim = rel_end;
  q.active = q.b0 < rel_end;
  q.last_active = (int)((bits - 1u + S) / sb);
  return q;
}

// k_row_count's record of one lane of a row (see decode_stream's pre_start / pre_off),
// in registers.
struct PreLane {
  uint32_t start, off, nxt, tot, endrel, valid, rounds;
  uint32_t nstart;   // the right neighbour's start (~0u: none, the lane walks to the end of the chunk)
};

// The fixpoint of a chunk that no count kernel has recorded, out of line: the row kernels reach
// it only for rows of several chunks or with an unusable record, and inlined its loops (and the
// 1024-lane scan behind them) were where most of those kernels' scalar registers went -- 47 to
// 118 SGPRs spilled to VGPR lanes, some reloaded inside the write loops.  Everything crosses
// the call by value (a reader passed by reference would live in scratch).
struct ColdFix { uint32_t start, endpos, cnt, rounds; unsigned long long off, tot; long long c_first; };
__device__ __attribute__((noinline)) ColdFix cold_fixpoint(const uint8_t *p, uint32_t stream_size,
                                                           unsigned long long abs_bit, const uint32_t *grp_lds,
                                                           const uint32_t *nd_lds, StreamShared *sh, bool active,
                                                           uint32_t lim, uint32_t start, uint32_t lead_bits) {
  GrpTables tb;
  tb.grp = reinterpret_cast<const uint2 *>(grp_lds); tb.gx = nullptr; tb.gy = nullptr; tb.nd = nd_lds;
  GReader rd;
  const uint32_t rel0 = rd.attach(p, stream_size, abs_bit);
  ColdFix r;
  r.start = start; r.endpos = start; r.cnt = 0; r.rounds = 0; r.c_first = 0;
  lean_fixpoint(rd, tb, sh, rel0, active, lim, &r.start, &r.endpos, &r.cnt, &r.rounds, false, lead_bits, &r.c_first);
  r.off = block_scan_u64(r.cnt, sh->sm64, &r.tot);
  return r;
}

// Decode one whole stream with one workgroup, chunk after chunk (each chunk's
// first token position is exact because the previous chunk has finished).  The
// sub-sequence length is chosen so that the 1024 lanes cover the remaining payload
// (one chunk, normally).
// FUSED: the whole output (out_size bytes) lives in LDS at `lds_out` (pre-zeroed
// by the caller) and the bytes are OR-ed in there; otherwise they go through the
// LDS window `win` to `gout`.  Returns (to every lane) 0 when the stream is
// accepted like UncompressStream accepts it (huffman_dec.cpp:361-417).
// pre_start / pre_off (optional): the fixpoint of the stream's single chunk computed
// beforehand by k_row_count (pre_off[kDecThreads + 2] != 0 says it is usable).
// GLOBAL (with FUSED false): the output goes straight to `gout`, PRE-ZEROED global
// memory, without the LDS window (win may be nullptr) -- the LRES serial fallback.
// PRIMED: the caller has set sh->err / sh->endbit in front of a barrier of its own.
template <bool FUSED, bool GLOBAL = false, bool PRIMED = false>
__device__ __forceinline__ int decode_stream(const uint8_t *p, uint32_t stream_size, uint32_t pay_off,
                             uint32_t pay_len, uint32_t out_size, const GrpTables &tb,
                             StreamShared *sh, uint8_t *lds_out, uint32_t *win, uint8_t *gout,
                             uint32_t *stats, uint32_t max_sub, uint32_t lead_bits,
                             const uint32_t *pre_start = nullptr, const uint32_t *pre_off = nullptr) {
  const int tid = threadIdx.x;
  if (!PRIMED) {
    if (tid == 0) { sh->err = 0; sh->endbit = ~0ull; }
    __syncthreads();
  }

  const unsigned long long P1 = 8ull * pay_len;  // payload end, in bits from pay_off
  unsigned long long cur = 0;                    // exact bit position of the next token
  unsigned long long O0 = 0;                     // symbols produced so far
  uint32_t st_chunks = 0, st_rounds = 0;
  long long c_sync = 0, c_write = 0, c_r1 = 0, c_t0 = clock64();
  bool synced = false;   // (uniform) a barrier stands between the last write pass and here

  while (cur < P1 && O0 < out_size) {
    synced = false;
    GReader rd;
    const uint32_t rel0 = rd.attach(p, stream_size, 8ull * pay_off + cur);
    ++st_chunks;

    const unsigned long long rem = P1 - cur;
    uint32_t sub = (uint32_t)((rem + kDecThreads - 1) / kDecThreads);
    sub = (sub + 31u) & ~31u;
    sub = sub < kMinSubBits ? kMinSubBits : (sub > max_sub ? max_sub : sub);
    const unsigned long long chunk_bits = (unsigned long long)sub * kDecThreads;
    const uint32_t rel_end = rel0 + (uint32_t)(rem < chunk_bits ? rem : chunk_bits);
    const SubGrid sg = sub_grid(rel0, rel_end - rel0, sub, tid);
    const uint32_t my_b0 = sg.b0, lim = sg.lim;
    const bool active = sg.active;
    const int last_active = sg.last_active;

    uint32_t start = active ? my_b0 : rel_end, endpos = start, cnt = 0;
    unsigned long long tot, off;
    // Where the lane's walk ends.  With k_row_count's records: at its right neighbour's
    // start -- the count kernels divide the chunk at token boundaries of their own choice
    // (k_row_count_w: the first GROUP boundary at or past the nominal one), and a lane
    // owns exactly the tokens in front of its neighbour's first.
    uint32_t wlim = lim;
    const uint32_t pre_valid = cur != 0 ? 0u : pre_off ? pre_off[kDecThreads + 2] : 0u;
    const bool pre = pre_valid != 0, chain = pre_valid == 3u;
    if (pre) {
      const uint32_t ns = tid + 1 < kDecThreads ? pre_start[tid + 1] : ~0u;
      wlim = ns < rel_end - rel0 ? rel0 + ns : rel_end;
    }
    if (pre) {
      // One chunk, fixpoint done by k_row_count at twice the occupancy.
      start = rel0 + pre_start[tid];
      off = pre_off[tid];
      const uint32_t nxt_off = pre_off[tid + 1];   // [kDecThreads] holds the total
      cnt = nxt_off - (uint32_t)off;
      tot = pre_off[kDecThreads];
      if (tid == last_active) endpos = rel0 + pre_off[kDecThreads + 1];
      st_rounds += pre_off[kDecThreads + 3];
    } else {
      const ColdFix cf = cold_fixpoint(p, stream_size, 8ull * pay_off + cur, reinterpret_cast<const uint32_t *>(tb.grp),
                                       tb.nd, sh, active, lim, start, lead_bits);
      start = cf.start; endpos = cf.endpos; cnt = cf.cnt; st_rounds += cf.rounds;
      c_r1 += cf.c_first; off = cf.off; tot = cf.tot;
    }
    { const long long t = clock64(); c_sync += t - c_t0; c_t0 = t; }

    const unsigned long long opl = O0 + off;
    // The lane in whose range the block completes takes the exact path.
    const bool inside = opl + cnt < out_size, exact = !inside && opl < out_size;
    if (FUSED) {
      uint32_t end_bp = ~0u;
      if (inside) {
        if (!lean_write(rd, tb, start, wlim, (uint32_t)opl, lds_out, 0u, chain)) sh->err = 1;
      } else if (exact) {
        if (!exact_write(rd, tb, start, wlim, (uint32_t)opl, out_size, lds_out, &end_bp)) sh->err = 1;
      }
      if (end_bp != ~0u) sh->endbit = cur + (end_bp - rel0);
      __syncthreads();
    } else if (GLOBAL) {
      lean_write_global(rd, tb, sh, start, wlim, opl, exact, out_size, cur, rel0, gout, exact ? opl : opl + cnt);
      __syncthreads();
    } else {
      const unsigned long long O1 = (O0 + tot < out_size) ? O0 + tot : out_size;
      lean_write_windows(rd, tb, sh, start, wlim, opl, exact, O0, O1, out_size, cur, rel0, win, gout);
    }
    { const long long t = clock64(); c_write += t - c_t0; c_t0 = t; }

    // ---- advance to the next chunk ----
    if (tid == last_active) sh->nxt[0] = endpos;
    __syncthreads();
    const uint32_t last_end = sh->nxt[0];
    cur += (unsigned long long)(last_end - rel0);
    O0 += tot;
    if (last_end == rel0) break;  // no progress (cannot happen on a valid stream)
    __syncthreads();
  }
  if (!synced) __syncthreads();

  // ---- accept / reject like UncompressStream (huffman_dec.cpp:361-417) ----
  int bad = sh->err;
  if (O0 < out_size) bad = 1;  // ran out of payload before the block was full
  const unsigned long long E = sh->endbit;
  // AtTheEnd (huffman_dec.cpp:140-145): inside the payload's last byte, or exactly at its end.
  if (!bad && !(E <= P1 && E + 8 > P1 && E > 0)) bad = 1;
  if (tid == 0 && stats) {
    stats[0] = st_chunks; stats[1] = st_rounds;
    if (!FUSED) { stats[2] = 0; stats[3] = (uint32_t)(c_r1 >> 4); }   // fused: the caller's slots
    stats[4] = (uint32_t)(c_sync >> 4); stats[5] = (uint32_t)(c_write >> 4);
    stats[6] = pay_len; stats[7] = out_size;
  }
  return bad;
}

// The row kernel's normal case (4096-pixel rows): ONE chunk whose lanes a count kernel has
// recorded, the record in registers (PreLane).  Nothing of the sub-sequence grid is needed -- a
// lane walks from its recorded start to its right neighbour's -- and where the chunk ends is in
// the record as well: one barrier, behind the write pass.  Returns decode_stream's verdict, or
// -1 (to every lane, before anything is written) when the record is not usable: the caller
// then takes decode_stream_fused_cold.  The caller has set sh->err / sh->endbit in front of a
// barrier of its own (decode_stream's PRIMED).
__device__ __forceinline__ int decode_row_recorded(const uint8_t *p, uint32_t stream_size, uint32_t pay_off,
                                                   uint32_t pay_len, uint32_t out_size, const GrpTables &tb,
                                                   StreamShared *sh, uint8_t *lds_out, uint32_t *stats,
                                                   const PreLane &pl) {
  const int tid = threadIdx.x;
  const unsigned long long P1 = 8ull * pay_len;
  if (pl.valid == 0 || P1 == 0 || out_size == 0) return -1;
  const long long c_t0 = clock64();
  GReader rd;
  const uint32_t rel0 = rd.attach(p, stream_size, 8ull * pay_off);
  const uint32_t rel_end = rel0 + (uint32_t)P1;   // (a recorded row is one chunk: k_row_count)
  const uint32_t start = rel0 + pl.start, opl = pl.off, cnt = pl.nxt - pl.off;
  const uint32_t wlim = pl.nstart < (uint32_t)P1 ? rel0 + pl.nstart : rel_end;
  const bool inside = opl + cnt < out_size, exact = !inside && opl < out_size;
  uint32_t end_bp = ~0u;
  if (inside) {
    if (!lean_write(rd, tb, start, wlim, opl, lds_out, 0u, pl.valid == 3u)) sh->err = 1;
  } else if (exact) {
    if (!exact_write(rd, tb, start, wlim, opl, out_size, lds_out, &end_bp)) sh->err = 1;
  }
  if (end_bp != ~0u) sh->endbit = (unsigned long long)(end_bp - rel0);
  __syncthreads();
  const long long c_t1 = clock64();
  // ---- accept / reject like UncompressStream (huffman_dec.cpp:361-417) ----
  int bad = sh->err;
  if (pl.tot < out_size) bad = 1;  // ran out of payload before the block was full
  const unsigned long long E = sh->endbit;
  // AtTheEnd (huffman_dec.cpp:140-145): inside the payload's last byte, or exactly at its end.
  if (!bad && !(E <= P1 && E + 8 > P1 && E > 0)) bad = 1;
  if (tid == 0 && stats) {
    stats[0] = 1; stats[1] = pl.rounds;
    stats[4] = 0; stats[5] = (uint32_t)((c_t1 - c_t0) >> 4);
    stats[6] = pay_len; stats[7] = out_size;
  }
  return bad;
}

// A row without a usable record (several chunks, a count kernel that gave up): the general
// decoder, OUT OF LINE -- inlined beside the fast path above it was most of the row kernel's
// code and of its scalar register pressure.  Everything crosses the call by value.
__device__ __attribute__((noinline)) int decode_stream_fused_cold(const uint8_t *p, uint32_t stream_size,
                                                                  uint32_t pay_off, uint32_t pay_len, uint32_t out_size,
                                                                  const uint32_t *grp_lds, const uint32_t *nd_lds,
                                                                  StreamShared *sh, uint8_t *lds_out, uint32_t *stats,
                                                                  uint32_t max_sub, uint32_t lead_bits) {
  GrpTables tb;
  tb.grp = reinterpret_cast<const uint2 *>(grp_lds); tb.gx = nullptr; tb.gy = nullptr; tb.nd = nd_lds;
  return decode_stream<true, false, true>(p, stream_size, pay_off, pay_len, out_size, tb, sh, lds_out, nullptr, nullptr,
                                          stats, max_sub, lead_bits);
}

// Tree nodes and decode tables of stream `strm` of frame f -> LDS.
__device__ __forceinline__ void load_dec_tables(const DecWs &ws, const DecFrame *df, int f, int strm,
                                                LdsTables *T) {
  const uint32_t *nodes = ws.nodes + ((size_t)f * 2 + strm) * (kMaxNodes + 1);
  const int nn = min(df->s[strm].num_nodes, kMaxNodes + 1);   // (a frame that failed to parse holds anything)
  for (int k = threadIdx.x; k < nn; k += kDecThreads) T->nd[k] = nodes[k];
  const uint4 *gg = reinterpret_cast<const uint4 *>(ws.grp + ((size_t)f * 2 + strm) * (1u << kLutBits));
  for (int k = threadIdx.x; k < (1 << kLutBits) / 2; k += kDecThreads)
    reinterpret_cast<uint4 *>(T->grp)[k] = gg[k];
  const uint4 *gs = reinterpret_cast<const uint4 *>(ws.sub + ((size_t)f * 2 + strm) * kSubEntries);
  for (int k = threadIdx.x; k < kSubEntries / 2; k += kDecThreads)
    reinterpret_cast<uint4 *>(T->grp + (1 << kLutBits))[k] = gs[k];
}

// ---------------------------------------------------------------------------
// k_dec_huff: generic stream decode to the symbol buffers in HBM.  Block 0 of a
// frame is its LRES stream; blocks 1.. are FRES block rows (only launched for
// rows that do not fit the fused kernel's LDS budget).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kDecThreads) void k_dec_huff(Geom g, DecWs ws, const uint8_t *packed,
                                                          size_t in_stride, const uint32_t *sizes,
                                                          int first_block, int lres_fallback_only,
                                                          int use_row_count) {
  __shared__ uint32_t win[kWinBytes / 4 + 1];
  __shared__ LdsTables T;
  __shared__ StreamShared sh;

  const int blk = blockIdx.x + first_block, f = blockIdx.y;
  DecFrame *df = ws.frames + f;
  // One read for the whole workgroup (other workgroups flag the frame concurrently;
  // a per-lane read could let some waves leave ahead of the barriers below).
  if (threadIdx.x == 0) sh.flag = df->status;
  __syncthreads();
  if (sh.flag) return;
  const int strm = blk == 0 ? 0 : 1;
  if (strm == 0 && lres_fallback_only && ws.ver_ok[f]) return;  // parallel LRES path succeeded
  const uint8_t *p = packed + (size_t)f * in_stride;
  uint32_t pay_off, pay_len, out_size;
  uint8_t *out;
  const uint32_t *pre_start = nullptr, *pre_off = nullptr;   // k_row_count's fixpoint, if it ran
  if (strm == 0) {
    pay_off = df->s[0].payload_off;
    pay_len = df->s[0].chunk_end - pay_off;
    out_size = (uint32_t)g.lres_size;
    out = ws.lres_sym + (size_t)f * ws.lres_stride;
  } else {
    const int r = blk - 1;
    pay_off = ws.row_off[(size_t)f * g.rows + r];
    pay_len = ws.row_len[(size_t)f * g.rows + r];
    out_size = (uint32_t)g.row_block;
    out = ws.fres_sym + (size_t)f * ws.fres_stride + (size_t)r * g.row_block;
    if (use_row_count) {
      pre_start = ws.lane_start + ((size_t)f * g.rows + r) * kDecThreads;
      pre_off = ws.lane_off + ((size_t)f * g.rows + r) * (kDecThreads + kRecHdr);
      // use_row_count == 2: rows with a usable fixpoint were written by k_row_window.
      if (use_row_count == 2 && pre_off[kDecThreads + 2] != 0) return;
    }
  }
  load_dec_tables(ws, df, f, strm, &T);
  __syncthreads();
  const GrpTables tb = tables_of(&T);
  const int bad = decode_stream<false>(p, sizes[f], pay_off, pay_len, out_size, tb, &sh, nullptr, win,
                                       out, ws.stats + ((size_t)f * (g.rows + 1) + blk) * 8,
                                       (uint32_t)g.max_sub, (uint32_t)g.lead_bits, pre_start, pre_off);
  if (bad && threadIdx.x == 0) atomicMax(&df->status, fmt_err(strm == 0 ? 4 : 7, 1));
}

// ---------------------------------------------------------------------------
// Parallel LRES decode.  The LRES payload is ONE Huffman stream (~1 M symbols at
// 4096x4096), a long pole for a single workgroup.  All of its chunks are decoded
// speculatively in parallel and the chain between chunks is then made exact:
//   k_lres_spec    chunk k assumes its first token starts at its nominal first
//                  bit and runs the in-chunk fixpoint; stores every lane's start,
//                  end and symbol count, the chunk's end position and total.
//   k_lres_fix     one workgroup per frame: chunk k (k >= 1) is re-based on
//                  T_k = spec end of chunk k-1 -- by one sub-sequence of work when
//                  the chain re-joins the speculative one at once (the normal case),
//                  by a WARM restart of the chunk's fixpoint otherwise -- and the
//                  chain of ends is verified (see the kernel).
//   k_lres_write   chunk k writes its symbols from the corrected lane starts.
// If an end did change (a mis-speculation ran through a whole 32 KiB chunk) the
// frame falls back to the serial workgroup-per-stream path (k_dec_huff).
// ---------------------------------------------------------------------------
constexpr int kLresChunkBits = kDecThreads * kLresSubBits;

// One chunk of the LRES stream, tables already in LDS.  FIX false: the speculative
// in-chunk fixpoint from the nominal first bit.  FIX true: the warm restart with lane
// 0 at T = the speculative end of the previous chunk (the caller has established that
// the cheap test failed).
// The chunk's payload is staged in LDS first (s_pay, kLresPayWords dwords): the rounds
// of a chain that does not self-synchronise -- the run tokens of a constant plane, e.g.
// opaque alpha, repeat with a period and keep a wrong phase for their whole length --
// are ONE lane decoding one sub-sequence each, i.e. pure load latency, and that of the
// LDS is a tenth of the L2's.
constexpr int kLresPayWords = kDecThreads * kLresSubBits / 32 + 8;
constexpr int kLresMemo = kLresMemoWords;   // starts a lane remembers
template <bool FIX>
__device__ __forceinline__ void lres_chain_body(const Geom &g, const DecWs &ws, const uint8_t *p, uint32_t stream_size,
                                const DecFrame *df, int f, int k, const GrpTables &tb, StreamShared *sh,
                                uint32_t *s_pay) {
  const int tid = threadIdx.x;
  const uint32_t pay_off = df->s[0].payload_off;
  const unsigned long long P1 = 8ull * (df->s[0].chunk_end - pay_off);
  const unsigned long long cur = (unsigned long long)k * kLresChunkBits;
  const size_t slot = (size_t)f * ws.lres_chunks + k;
  uint64_t *end_out = FIX ? ws.fix_end : ws.spec_end;
  GReader gr;
  const uint32_t rel0 = gr.attach(p, stream_size, 8ull * pay_off + cur);
  LReader rd;
  // Bits up to rel0 + chunk + 46 are consumed and the reader runs three dwords ahead:
  // all inside the staged words, the clamp at jmax is never the stream's data.
  stage_payload(gr, s_pay, (uint32_t)kLresPayWords);
  __syncthreads();
  rd.w = (const __attribute__((address_space(3))) uint32_t *)s_pay;
  rd.jmax = kLresPayWords - 1;
  const unsigned long long rem = P1 - cur;
  const uint32_t rel_end = rel0 + (uint32_t)(rem < (unsigned long long)kLresChunkBits ? rem : kLresChunkBits);
  const uint32_t my_b0 = rel0 + tid * kLresSubBits;
  uint32_t lim = my_b0 + kLresSubBits;
  if (lim > rel_end) lim = rel_end;
  const bool active = my_b0 < rel_end;
  const int last_active = (int)((rel_end - rel0 - 1u) / kLresSubBits);
  uint32_t start = active ? my_b0 : rel_end, endpos = start, cnt = 0, rounds = 0, first = rel0;
  if (FIX) {
    const unsigned long long T = ws.spec_end[slot - 1];
    // A token is at most 46 bits, so the true first token lies in lane 0's range.
    if (T < cur || T >= cur + kLresSubBits) {
      if (tid == 0) ws.fix_end[slot] = ~0ull;  // forces the serial path
      return;
    }
    first = rel0 + (uint32_t)(T - cur);
    start = rel0 + ws.spec_start[slot * kDecThreads + tid];
    endpos = rel0 + ws.spec_endpos[slot * kDecThreads + tid];
    cnt = ws.spec_cnt[slot * kDecThreads + tid];
  }
  // The lane's memo (lean_fixpoint), handed from the speculative pass to the correction
  // through ws.spec_memo, one packed word per entry: start - nominal (<= 46: the
  // previous lane's last token) | end - lim (<= 46) << 6 | symbols (< 2^20) << 12.
  // Lane 0's start is given, it has no use for one.
  uint32_t memo[3 * kLresMemo];
  uint32_t *gm = ws.spec_memo + (slot * kDecThreads + tid) * kLresMemo;
#pragma unroll
  for (int e = 0; e < kLresMemo; ++e) {
    memo[3 * e] = ~0u; memo[3 * e + 1] = memo[3 * e + 2] = 0;
    if (FIX && tid > 0) {
      const uint32_t m = gm[e];
      if (m != ~0u) { memo[3 * e] = my_b0 + (m & 63u); memo[3 * e + 1] = lim + ((m >> 6) & 63u); memo[3 * e + 2] = m >> 12; }
    }
  }
  const long long c_in = clock64();
  lean_fixpoint<false, LReader, kLresMemo>(rd, tb, sh, first, active, lim, &start, &endpos, &cnt, &rounds, FIX,
                                           (uint32_t)g.lead_bits, nullptr, nullptr, memo);
  const long long c_fix = clock64() - c_in;
  if (!FIX) {
#pragma unroll
    for (int e = 0; e < kLresMemo; ++e) {
      const uint32_t ds = memo[3 * e] - my_b0, de = memo[3 * e + 1] - lim;
      gm[e] = (memo[3 * e] == ~0u || tid == 0 || ds > 46u || de > 46u || memo[3 * e + 2] >= (1u << 20))
                  ? ~0u : (ds | (de << 6) | (memo[3 * e + 2] << 12));
    }
  }
  unsigned long long tot;
  block_scan_u64(cnt, sh->sm64, &tot);
  ws.spec_start[slot * kDecThreads + tid] = start - rel0;
  ws.spec_endpos[slot * kDecThreads + tid] = endpos - rel0;
  ws.spec_cnt[slot * kDecThreads + tid] = cnt;
  if (tid == last_active) { end_out[slot] = cur + (endpos - rel0); ws.spec_tot[slot] = tot; }
  if (tid == 0) {
    uint32_t *st = ws.stats + ((size_t)f * (g.rows + 1)) * 8;
    atomicAdd(&st[FIX ? 2 : 0], 1u);
    atomicAdd(&st[FIX ? 3 : 1], rounds);
    atomicMax(&st[FIX ? 5 : 4], rounds);   // the slowest chunk sets the kernel's duration
    atomicMax(&st[FIX ? 7 : 6], (uint32_t)(c_fix >> 4));
  }
}

// k_lres_spec: every chunk of every frame, speculatively, in parallel.
__global__ __launch_bounds__(kDecThreads) void k_lres_spec(Geom g, DecWs ws, const uint8_t *packed,
                                                           size_t in_stride, const uint32_t *sizes) {
  __shared__ LdsTables T;
  __shared__ StreamShared sh;
  __shared__ __attribute__((aligned(16))) uint32_t s_pay[kLresPayWords];
  const int k = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  DecFrame *df = ws.frames + f;
  if (tid == 0) sh.flag = df->status;
  __syncthreads();
  if (sh.flag) return;
  const unsigned long long P1 = 8ull * (df->s[0].chunk_end - df->s[0].payload_off);
  const unsigned long long cur = (unsigned long long)k * kLresChunkBits;
  const size_t slot = (size_t)f * ws.lres_chunks + k;
  if (cur >= P1) {
    if (tid == 0) { ws.spec_end[slot] = cur; ws.spec_tot[slot] = 0; }
    return;
  }
  load_dec_tables(ws, df, f, 0, &T);
  __syncthreads();
  const GrpTables tb = tables_of(&T);
  lres_chain_body<false>(g, ws, packed + (size_t)f * in_stride, sizes[f], df, f, k, tb, &sh, s_pay);
}

// k_lres_fix: correction and verification of ALL chunks of a frame by one workgroup.
//   1. lane k = chunk k.  Chunk k's true first token starts where chunk k-1's
//      speculative chain ended (T); lane k decodes the first sub-sequence of its chunk
//      from T, and if that ends where the speculative first lane ended, nothing else in
//      the chunk changes: the chunk is settled with one sub-sequence of work (this
//      used to cost a whole workgroup and a load of the decode tables per chunk);
//   2. the chunks that did not re-join (none, normally) take the warm restart, one
//      after the other, with the whole workgroup;
//   3. chunk 0 is exact, so T_1 and hence chunk 1's corrected chain are exact; T_2 was
//      taken from chunk 1's SPECULATIVE end, which is right iff the correction left
//      that end unchanged -- and so on.  All ends unchanged => every chunk exact
//      (induction).  Output offsets = scan of the corrected totals.
__global__ __launch_bounds__(kDecThreads) void k_lres_fix(Geom g, DecWs ws, const uint8_t *packed,
                                                          size_t in_stride, const uint32_t *sizes) {
  __shared__ LdsTables T;
  __shared__ StreamShared sh;
  __shared__ uint8_t s_pending[kDecThreads];
  __shared__ int s_bad;
  __shared__ __attribute__((aligned(16))) uint32_t s_pay[kLresPayWords];
  const int f = blockIdx.x, k = threadIdx.x;
  DecFrame *df = ws.frames + f;
  if (k == 0) { ws.ver_ok[f] = 0; ws.lres_endbit[f] = ~0ull; s_bad = 0; sh.flag = df->status; }
  s_pending[k] = 0;
  __syncthreads();
  if (sh.flag) return;
  const uint32_t pay_off = df->s[0].payload_off;
  const unsigned long long P1 = 8ull * (df->s[0].chunk_end - pay_off);
  const int nact = (int)((P1 + kLresChunkBits - 1) / kLresChunkBits);
  if (nact > ws.lres_chunks || nact > kDecThreads) return;  // ver_ok stays 0 -> serial path
  load_dec_tables(ws, df, f, 0, &T);
  __syncthreads();
  const GrpTables tb = tables_of(&T);
  const uint8_t *p = packed + (size_t)f * in_stride;
  const size_t slot = (size_t)f * ws.lres_chunks + k;
  const unsigned long long cur = (unsigned long long)k * kLresChunkBits;
  // ---- 1: the cheap test, all chunks at once
  if (k == 0) {
    ws.fix_end[slot] = ws.spec_end[slot];   // chunk 0 is exact already
  } else if (k < nact) {
    const unsigned long long T = ws.spec_end[slot - 1];
    bool settled = false;
    if (T >= cur && T < cur + kLresSubBits) {
      GReader rd;
      const uint32_t rel0 = rd.attach(p, sizes[f], 8ull * pay_off + cur);
      const unsigned long long rem = P1 - cur;
      uint32_t lim = rel0 + kLresSubBits;
      const uint32_t rel_end = rel0 + (uint32_t)(rem < (unsigned long long)kLresChunkBits ? rem : kLresChunkBits);
      if (lim > rel_end) lim = rel_end;
      uint32_t pos, c;
      lean_count(rd, tb, rel0 + (uint32_t)(T - cur), lim, &pos, &c);
      if (pos - rel0 == ws.spec_endpos[slot * kDecThreads]) {
        const unsigned long long oldc = ws.spec_cnt[slot * kDecThreads];
        ws.spec_start[slot * kDecThreads] = (uint32_t)(T - cur);
        ws.spec_cnt[slot * kDecThreads] = c;
        ws.spec_tot[slot] = ws.spec_tot[slot] - oldc + c;
        ws.fix_end[slot] = ws.spec_end[slot];
        settled = true;
        atomicAdd(&ws.stats[((size_t)f * (g.rows + 1)) * 8 + 2], 1u);
      }
    }
    if (!settled) s_pending[k] = 1;
  }
  __syncthreads();
  // ---- 2: warm restarts of what is left
  for (int q = 1; q < nact; ++q) {
    if (!s_pending[q]) continue;   // LDS: the same for every lane
    lres_chain_body<true>(g, ws, p, sizes[f], df, f, q, tb, &sh, s_pay);
    __syncthreads();
  }
  // ---- 3: verification and output offsets (other lanes' global writes of this
  // kernel are read below)
  __threadfence_block();
  __syncthreads();
  unsigned long long ntot = 0;
  if (k < nact) {
    ntot = ws.spec_tot[slot];
    // The next chunk was corrected against spec_end[k]; that is the true end of
    // chunk k iff the correction of chunk k did not move it.
    if (k + 1 < nact && ws.fix_end[slot] != ws.spec_end[slot]) s_bad = 1;
  }
  unsigned long long tot;
  const unsigned long long base = block_scan_u64(ntot, sh.sm64, &tot);
  if (k < nact) ws.ver_base[slot] = base;
  __syncthreads();
  if (k == 0) ws.ver_ok[f] = (s_bad || g.lres_serial) ? 0 : 1;
}

__global__ __launch_bounds__(kDecThreads) void k_lres_write(Geom g, DecWs ws, const uint8_t *packed,
                                                            size_t in_stride, const uint32_t *sizes) {
  __shared__ LdsTables T;
  __shared__ StreamShared sh;
  const int k = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  DecFrame *df = ws.frames + f;
  // Everything the common path reads from global memory is requested in front of the
  // first barrier (the verdict, the chunk's output base, the lane's start and count,
  // the tables), so that the round trips overlap: the kernel is a handful of dependent
  // round trips long and runs on an empty GPU in front of the row kernel.
  const size_t slot = (size_t)f * ws.lres_chunks + k;
  const unsigned long long O0 = ws.ver_base[slot];
  const uint32_t start_rel = ws.spec_start[slot * kDecThreads + tid];
  const unsigned long long cnt = ws.spec_cnt[slot * kDecThreads + tid];
  // One read for the whole workgroup (other kernels may flag the frame meanwhile).
  if (tid == 0) sh.flag = df->status ? 1 : (ws.ver_ok[f] ? 0 : 2);
  load_dec_tables(ws, df, f, 0, &T);
  __syncthreads();
  if (sh.flag == 1) return;
  if (sh.flag == 2) {
    // The chunk chain did not verify (a mis-speculation ran through a whole chunk, or
    // the test knob): this frame's LRES stream is decoded by ONE workgroup, chunk
    // after chunk, every chunk starting at the exact end of the one before.
    if (k != 0) return;
    const GrpTables tb0 = tables_of(&T);
    const uint32_t po = df->s[0].payload_off;
    const int bad = decode_stream<false, true>(packed + (size_t)f * in_stride, sizes[f], po, df->s[0].chunk_end - po,
                                               (uint32_t)g.lres_size, tb0, &sh, nullptr, nullptr,
                                               ws.lres_sym + (size_t)f * ws.lres_stride,
                                               ws.stats + ((size_t)f * (g.rows + 1)) * 8, (uint32_t)g.max_sub,
                                               (uint32_t)g.lead_bits);
    if (bad && tid == 0) atomicMax(&df->status, fmt_err(4, 1));
    return;
  }
  const uint32_t pay_off = df->s[0].payload_off;
  const unsigned long long P1 = 8ull * (df->s[0].chunk_end - pay_off);
  const unsigned long long cur = (unsigned long long)k * kLresChunkBits;
  if (cur >= P1) return;
  const uint32_t out_size = (uint32_t)g.lres_size;
  if (O0 >= out_size) return;
  if (tid == 0) { sh.err = 0; sh.endbit = ~0ull; }
  const GrpTables tb = tables_of(&T);
  GReader rd;
  const uint32_t rel0 = rd.attach(packed + (size_t)f * in_stride, sizes[f], 8ull * pay_off + cur);
  const unsigned long long rem = P1 - cur;
  const uint32_t rel_end = rel0 + (uint32_t)(rem < (unsigned long long)kLresChunkBits ? rem : kLresChunkBits);
  uint32_t lim = rel0 + (tid + 1) * kLresSubBits;
  if (lim > rel_end) lim = rel_end;
  const uint32_t start = rel0 + start_rel;
  __syncthreads();
  unsigned long long tot;
  const unsigned long long off = block_scan_u64(cnt, sh.sm64, &tot);
  const unsigned long long opl = O0 + off;
  const bool exact = !(opl + cnt < out_size) && opl < out_size;
  // The symbols were zeroed by launch_decode: only non-zero literals are stored.
  lean_write_global(rd, tb, &sh, start, lim, opl, exact, out_size, cur, rel0,
                    ws.lres_sym + (size_t)f * ws.lres_stride, exact ? opl : opl + cnt);
  __syncthreads();
  if (tid == 0) {
    if (sh.err) atomicMax(&df->status, fmt_err(4, 1));
    if (sh.endbit != ~0ull) ws.lres_endbit[f] = sh.endbit;
  }
}

// Accept / reject the LRES stream like UncompressStream (huffman_dec.cpp:361-417).
__global__ void k_lres_finish(DecWs ws, int batch) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= batch) return;
  DecFrame *df = ws.frames + f;
  if (df->status || !ws.ver_ok[f]) return;  // failed earlier, or handled by the serial path
  const unsigned long long P1 = 8ull * (df->s[0].chunk_end - df->s[0].payload_off);
  const unsigned long long E = ws.lres_endbit[f];
  if (!(E != ~0ull && E <= P1 && E + 8 > P1 && E > 0)) atomicMax(&df->status, fmt_err(4, 1));
}

// ---------------------------------------------------------------------------
// k_lres_unpredict: one wavefront per 16x16 macro block, anti-diagonal
// wavefronts like k_lres_predict (downsampled.cpp:318-382).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int predict_d(int s1, int s2, int s3, int p) {
  switch (p) {
    default:
    case 0: return clamp255d((3 * (s2 + s3) - 2 * s1 + 2) >> 2);
    case 1: return s2;
    case 2: return s3;
    case 3: return (s2 + s3 + 1) >> 1;
    case 4: return clamp255d(s2 + s3 - s1);
  }
}

// LDS exchange inside ONE wavefront: its LDS operations execute in order, so the
// fences only keep the compiler from moving them.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sixteen macro blocks per workgroup: four wavefronts, each on its own (four blocks of
// 16 lanes, see k_lres_predict) -- one-wavefront workgroups made this kernel a test of
// the dispatcher (65 536 workgroups for 64 frames of 4096 x 4096), and it sits on the
// critical path between k_row_count and the row kernel.
constexpr int kUnpredWaves = 4;
__global__ __launch_bounds__(64 * kUnpredWaves) void k_lres_unpredict(Geom g, DecWs ws) {
  __shared__ uint8_t rec_s[kUnpredWaves][4][17][18];   // the reconstructed blocks with a border row / column in front
  __shared__ uint8_t dl_s[kUnpredWaves][4][16][16];   // the blocks' deltas: the chain below reads one per step
  __shared__ int16_t s_lmap[128];   // the chain below looks a delta up per step: LDS, not global
  __shared__ int s_status;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = lane >> 4, dv = lane & 15;
  uint8_t (*rec)[17][18] = rec_s[wv];
  uint8_t (*dl)[16][16] = dl_s[wv];
  const int mu = (blockIdx.x * kUnpredWaves + wv) * 4 + b, mv = blockIdx.y;
  const int f = blockIdx.z / g.C, c = blockIdx.z % g.C;
  const DecFrame *df = ws.frames + f;
  if (threadIdx.x == 0) s_status = df->status;
  if (threadIdx.x < 128) s_lmap[threadIdx.x] = df->lmap[threadIdx.x];
  const uint8_t *in = ws.lres_sym + (size_t)f * ws.lres_stride + (size_t)c * g.chan_size;
  uint8_t *m = ws.low + (size_t)f * ws.plane_stride + (size_t)c * g.rows * g.cols;
  const bool live = mu < g.mcols;
  const int u0 = mu * 16, v0 = mv * 16;
  const int bw = live ? min(16, g.cols - u0) : 0, bh = min(16, g.rows - v0);
  // DecodePredictor (downsampled.cpp:37-39): uint8 + 2 in int arithmetic, so
  // stored 254/255 come back as 256/257 and fall into PredictSample's default.
  const int pc = live ? (int)in[mv * g.mcols + mu] + 2 : 0;
  const uint8_t *src = in + g.mrows * g.mcols + (size_t)v0 * g.cols + (size_t)bh * u0;
  // The lane's row of deltas goes to LDS up front (sixteen loads in flight at once)
  // instead of one dependent global load per step of the chain.
  if (dv < bh) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < bw) dl[b][dv][k] = src[dv * bw + k];
  }
  __syncthreads();
  if (s_status) return;
  // The chain, branch free (as k_lres_predict's): neighbours from a copy of the block with a border
  // (index + 1), the edge cases of downsampled.cpp:318-382 as four selects, all predictors computed
  // and the block's selected -- the four blocks of a wavefront use different ones.
  const bool row_live = dv < bh, up_ok = dv > 0;
  uint8_t *rrow = &rec[b][dv + 1][1];          // rrow[du] = reconstructed sample (dv, du)
  const uint8_t *urow = &rec[b][dv][1];        // the row above
  uint8_t *mrow = m + (size_t)(v0 + dv) * g.cols + u0;
  for (int d = 0; d < 31; ++d) {
    const int du = d - dv;
    const bool active = row_live && du >= 0 && du < bw;
    const int duc = active ? du : 0;
    const int left = rrow[duc - 1], up = urow[duc], ul = urow[duc - 1];
    const bool left_ok = duc > 0;
    const int f = up_ok ? up : (left_ok ? left : 128);
    const int s3 = left_ok ? left : f, s2 = f, s1 = (up_ok && left_ok) ? ul : f;
    const int t = s2 + s3;
    const int p0 = clamp255d((3 * t - 2 * s1 + 2) >> 2), p3 = (t + 1) >> 1, p4 = clamp255d(t - s1);
    const int predicted = pc == 1 ? s2 : pc == 2 ? s3 : pc == 3 ? p3 : pc == 4 ? p4 : p0;
    const int sc = (int8_t)dl[b][dv][duc];
    // mapper.h:33-35 with the mirrored table (mapper.cpp:148-154).
    const int mag = s_lmap[sc < 0 ? (sc == -128 ? 127 : -sc) : sc];
    const int un = sc < 0 ? -mag : mag;
    const int val = clamp255d((int)(int16_t)(predicted + un));
    if (active) {
      rrow[du] = (uint8_t)val;
      mrow[du] = (uint8_t)val;
    }
    wave_lds_sync();   // (the exchange is inside the wavefront)
  }
}

// ---------------------------------------------------------------------------
// Inverse transform (shared by k_dec_row_fused and k_tile_inv).
// ---------------------------------------------------------------------------
// Inverse 8-point butterfly: int32, floor >>3, narrowed to int16 (hadamard.cpp:47-74).
__device__ __forceinline__ void iwht8(int &x0, int &x1, int &x2, int &x3, int &x4, int &x5,
                                      int &x6, int &x7) {
  const int a0 = x0 + x4, a1 = x1 + x5, a2 = x2 + x6, a3 = x3 + x7;
  const int a4 = x0 - x4, a5 = x1 - x5, a6 = x2 - x6, a7 = x3 - x7;
  const int b0 = a0 + a2, b1 = a1 + a3, b2 = a0 - a2, b3 = a1 - a3;
  const int b4 = a4 + a6, b5 = a5 + a7, b6 = a4 - a6, b7 = a5 - a7;
  x0 = (int16_t)((b0 + b1) >> 3); x1 = (int16_t)((b4 + b5) >> 3);
  x2 = (int16_t)((b6 + b7) >> 3); x3 = (int16_t)((b2 + b3) >> 3);
  x4 = (int16_t)((b2 - b3) >> 3); x5 = (int16_t)((b6 - b7) >> 3);
  x6 = (int16_t)((b4 - b5) >> 3); x7 = (int16_t)((b0 - b1) >> 3);
}

// ---------------------------------------------------------------------------
// k_dec_row_fused: one 1024-lane workgroup per FRES block row, when the row's
// symbols fit in LDS (row_block <= ~128 KiB, i.e. width <= 4096 for RGBA).
//   1. entropy-decode the row into LDS (decode_stream<true>);
//   2. lane = tile: gather, dequantise, inverse WHT, + low-res, clamp; results
//      overwrite the tile's own 64 symbol slots per channel (in place);
//   3. lane = (tile, pixel row): colour inverse and two 16-byte stores, so a wave
//      writes 2 KiB of contiguous pixels per pixel row.
// The symbols never touch HBM: traffic is the packed row in, the pixels out.
// ---------------------------------------------------------------------------
struct FusedLayout {
  uint32_t sym, tab, sh, unmap, shift, shiftp, total;
};
__host__ __device__ inline FusedLayout fused_layout(int row_block, int rows = 1) {
  FusedLayout L;
  uint32_t o = 0;
  auto carve = [&](uint32_t bytes) { uint32_t r = o; o += (bytes + 15u) & ~15u; return r; };
  L.tab = carve((uint32_t)sizeof(LdsTables));   // at offset 0: the hot loop indexes it
  L.sym = carve((((uint32_t)row_block + 15u) & ~15u) * (uint32_t)rows);   // `rows` block rows of symbols
  L.sh = carve((uint32_t)sizeof(StreamShared));
  L.unmap = carve(512u);
  L.shift = carve(128u);
  L.shiftp = carve(256u + 16u);   // 2 x 32 packed shift pairs, then kHfast words (tile_plane's identity test)
  L.total = o;
  return L;
}

// ---------------------------------------------------------------------------
// Packed-int16 inverse transform of one 8x8 plane (one channel of one tile).
//
// The reference does every butterfly in int32 and narrows after the >>3
// (hadamard.cpp:47-74), so 16-bit lanes are only exact while no sum of eight
// terms leaves int16.  With every dequantised coefficient in [-4096, 4095] that
// holds for both passes (|sum| <= 32767 + the one -32768 that still fits, and a
// pass maps the range onto itself), which is the case for anything but
// synthetic full-swing noise; a plane with a larger coefficient takes the
// scalar int32 path below.  Both paths are bit-exact.
//
// Layout of the packed path: V[x*4 + j] = rows (2j, 2j+1) of column x, so the
// row pass (along x) is element-wise over registers; one v_perm per register
// pair turns that into T[y*4 + i] = columns (2i, 2i+1) of row y for the column
// pass (along y).  The bilinear low-res block (downsampled.cpp:116-169) is
// built four rows per register with v_lerp_u8 ((a + b + 1) >> 1 per byte), the
// int16 add + ClampTo8Bit (decoder.cpp:401-413) is pk_add + v_sat_pk_u8_i16.
// Output: O[y*2 + h] = the clamped bytes of row y, x = 4h..4h+3.
// ---------------------------------------------------------------------------
typedef short dpk16 __attribute__((ext_vector_type(2)));
typedef unsigned short dupk16 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t sat_pk_u8(uint32_t x) {
  uint32_t r;
  asm("v_sat_pk_u8_i16 %0, %1" : "=v"(r) : "v"(x));
  return r;   // byte 0 = sat(lo half), byte 1 = sat(hi half)
}

// The same into the HIGH half of `lo` (whose low half holds an earlier pair's two bytes): SDWA
// writes the result word there and keeps the other, which saves the v_perm that would merge
// two results.
__device__ __forceinline__ uint32_t sat_pk_u8_hi(uint32_t lo, uint32_t x) {
  asm("v_sat_pk_u8_i16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(lo) : "v"(x));
  return lo;
}

// 2 * a + c on packed int16 pairs, one instruction.
__device__ __forceinline__ uint32_t pk_mad2(dpk16 a, dpk16 c) {
  uint32_t r;
  asm("v_pk_mad_i16 %0, %1, 2, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, a)), "v"(__builtin_bit_cast(uint32_t, c)));
  return r;
}

__device__ __forceinline__ void iwht8_pk(dpk16 &x0, dpk16 &x1, dpk16 &x2, dpk16 &x3, dpk16 &x4,
                                         dpk16 &x5, dpk16 &x6, dpk16 &x7) {
  const dpk16 three = {3, 3};
  const dpk16 a0 = x0 + x4, a1 = x1 + x5, a2 = x2 + x6, a3 = x3 + x7;
  const dpk16 a4 = x0 - x4, a5 = x1 - x5, a6 = x2 - x6, a7 = x3 - x7;
  const dpk16 b0 = a0 + a2, b1 = a1 + a3, b2 = a0 - a2, b3 = a1 - a3;
  const dpk16 b4 = a4 + a6, b5 = a5 + a7, b6 = a4 - a6, b7 = a5 - a7;
  x0 = (b0 + b1) >> three; x1 = (b4 + b5) >> three;
  x2 = (b6 + b7) >> three; x3 = (b2 + b3) >> three;
  x4 = (b2 - b3) >> three; x5 = (b6 - b7) >> three;
  x6 = (b4 - b5) >> three; x7 = (b0 - b1) >> three;
}

// lerp tree of downsampled.cpp:116-169 on four packed bytes.
__device__ __forceinline__ void interp9_u8x4(uint32_t a[9]) {
  const uint32_t rnd = 0x01010101u;
  a[4] = __builtin_amdgcn_lerp(a[0], a[8], rnd);
  a[2] = __builtin_amdgcn_lerp(a[0], a[4], rnd);
  a[6] = __builtin_amdgcn_lerp(a[4], a[8], rnd);
  a[1] = __builtin_amdgcn_lerp(a[0], a[2], rnd);
  a[3] = __builtin_amdgcn_lerp(a[2], a[4], rnd);
  a[5] = __builtin_amdgcn_lerp(a[4], a[6], rnd);
  a[7] = __builtin_amdgcn_lerp(a[6], a[8], rnd);
}

// Low-res block: LQ[q][x] = bytes of rows 4q..4q+3 at column x.
__device__ __forceinline__ void lowres_quads(uint32_t lr0, uint32_t lr8, uint32_t LQ[2][8]) {
  uint32_t lr[9];
  lr[0] = lr0; lr[8] = lr8;
  interp9_u8x4(lr);   // bytes 0,1 = left,right of rows 0..7
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint32_t p01 = __builtin_amdgcn_perm(lr[4 * q + 1], lr[4 * q], 0x05010400u);      // L0 L1 R0 R1
    const uint32_t p23 = __builtin_amdgcn_perm(lr[4 * q + 3], lr[4 * q + 2], 0x05010400u);  // L2 L3 R2 R3
    uint32_t a[9];
    a[0] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
    a[8] = __builtin_amdgcn_perm(p23, p01, 0x07060302u);
    interp9_u8x4(a);
#pragma unroll
    for (int x = 0; x < 8; ++x) LQ[q][x] = a[x];
  }
}

// When are 16-bit lanes exact for the two inverse passes?  The reference adds in int32
// and narrows after each pass's >> 3 (hadamard.cpp:47-74), so all that is needed is
// that no butterfly sum leaves int16, i.e. sum |d| <= 32767 over every ROW going into
// the row pass and over every column of its results.  Two sufficient conditions on the
// dequantised coefficients, checked from running maxima / minima (v_pk_max_i16 /
// v_pk_min_i16):
//   (A) |d| <= 3071 everywhere but in register 0 (rows 0 and 1 of column 0: the DC and
//       its vertical neighbour), where |d| <= 11263:  rows 0, 1: 11263 + 7 x 3071 =
//       32760; other rows 8 x 3071; after >> 3 at most 4095 / 3071, so a column sums to
//       at most 2 x 4095 + 6 x 3071 = 26616;
//   (B) |d| <= 4095 everywhere (8 x 4095 = 32760 in both passes).
// (B) alone -- the round-2 test -- fails in nine of ten wavefronts of the benchmark
// frames, whose DC terms reach 8320 (alpha: 10448): a tile whose neighbours differ needs
// a large DC correction on top of the bilinear low-res plane, and ONE such lane sent its
// whole wavefront through the scalar int32 path as well.  (A) holds for every tile of
// those frames, (B) covers full-swing noise with small DC terms; a plane that satisfies
// neither takes the scalar path, which is exact for anything.
struct RangeAcc {
  dpk16 mx, mn;
  __device__ __forceinline__ void init() { mx = dpk16{-32768, -32768}; mn = dpk16{32767, 32767}; }
  __device__ __forceinline__ void add(dpk16 d) { mx = __builtin_elementwise_max(mx, d); mn = __builtin_elementwise_min(mn, d); }
};
__device__ __forceinline__ bool packed_wht_exact(const RangeAcc &others, dpk16 d0) {
  const dpk16 zero = {0, 0};
  const dupk16 am = __builtin_bit_cast(dupk16, (dpk16)__builtin_elementwise_max(others.mx, __builtin_elementwise_sub_sat(zero, others.mn)));
  const dupk16 a0 = __builtin_bit_cast(dupk16, (dpk16)__builtin_elementwise_max(d0, __builtin_elementwise_sub_sat(zero, d0)));
  const dupk16 t3071 = {3071, 3071}, t4095 = {4095, 4095}, t11263 = {11263, 11263};
  const uint32_t oa = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(am, t3071)) |
                      __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(a0, t11263));
  const uint32_t ob = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(am, t4095)) |
                      __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(a0, t4095));
  return oa == 0u || ob == 0u;
}

// slot: the tile's first symbol (scan index k is at slot[k * cols]); shift: the
// 64 per-position shifts; shiftp: the same as 32 packed pairs in V order; lr0 /
// lr8: (left, right) low-res samples of this and the next block row in bytes 0, 1.
// hfast (COLS != 0): {bias pair, mask pair} of the identity test below.
// COLS > 0: the tile count per block row at compile time (slot offsets are immediates);
// COLS < 0: the same fast gather with the run-time count (64 address adds per plane).
template <int COLS>
__device__ __forceinline__ void tile_plane(const uint8_t *slot, int cols_rt, const int16_t *s_unmap,
                                           const uint8_t *shift, const uint32_t *shiftp,
                                           uint32_t lr0, uint32_t lr8, uint32_t O[16],
                                           const uint32_t *hfast = nullptr) {
  const int cols = COLS > 0 ? COLS : cols_rt;
  // Gather + dequantise (quantize.cpp:153-165: int16 wrap == 16-bit shift left).
  dpk16 V[32];
  RangeAcc rng;
  rng.init();
  if (COLS != 0) {
    // The companding table is the identity for small codes (mapper.cpp:54-61: up to
    // 49 in the encoder's table; the decoder derives the range from the stream's
    // FMAP), and everything but the lowest frequencies of a tile IS small.  The 21
    // register pairs that hold rows 2..7 of columns 1..7 (group H) are therefore
    // loaded as sign-extended bytes straight into the packed halves
    // (ds_read_i8_d16 / _d16_hi: no look-up, no address arithmetic, no v_perm) and
    // tested ONCE per plane and wavefront: every code in [-B, B) with B a power of
    // two inside the identity range and B << (largest H shift) <= 2048, so the test
    // also stands for the 16-bit range check of these coefficients.  A wavefront
    // with a larger code in H takes the look-ups for H as well.  Group L (rows 0, 1
    // and column 0: the DC and first-order coefficients, large in most tiles)
    // always goes through the table.
    const uint32_t hb = hfast[0], hm = hfast[1];
    uint32_t W[32], hacc = 0;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      const int x = e >> 2, j = e & 3, p0 = (2 * j) * 8 + x;
      const uint8_t *q0 = slot + (size_t)kInvScanD[p0] * cols, *q1 = slot + (size_t)kInvScanD[p0 + 8] * cols;
      if (x == 0 || j == 0) {
        W[e] = (uint32_t)(uint16_t)s_unmap[*q0] | ((uint32_t)(uint16_t)s_unmap[*q1] << 16);
      } else {
        dpk16 w;
        w.x = (short)(int8_t)*q0;
        w.y = (short)(int8_t)*q1;
        W[e] = __builtin_bit_cast(uint32_t, w);
        hacc |= __builtin_bit_cast(uint32_t, (dupk16)(__builtin_bit_cast(dupk16, w) + __builtin_bit_cast(dupk16, hb)));
      }
    }
    const bool hslow = __any((hacc & hm) != 0u);
    if (__builtin_expect(hslow, 0)) {
#pragma unroll
      for (int e = 0; e < 32; ++e) {
        const int x = e >> 2, j = e & 3;
        if (x == 0 || j == 0) continue;
        W[e] = (uint32_t)(uint16_t)s_unmap[W[e] & 255u] | ((uint32_t)(uint16_t)s_unmap[(W[e] >> 16) & 255u] << 16);
      }
    }
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      const int x = e >> 2, j = e & 3;
      const dupk16 d = __builtin_bit_cast(dupk16, W[e]) << __builtin_bit_cast(dupk16, shiftp[e]);
      V[e] = __builtin_bit_cast(dpk16, d);
      if ((x == 0 || j == 0) && e != 0) rng.add(V[e]);   // (group H: below 2048 by its own test)
    }
    if (__builtin_expect(hslow, 0)) {
#pragma unroll
      for (int e = 0; e < 32; ++e) {
        const int x = e >> 2, j = e & 3;
        if (x == 0 || j == 0) continue;
        rng.add(V[e]);
      }
    }
  } else {
    uint32_t W[32];
    {
      // Run-time column count: walk the slots in scan order with one running
      // pointer (64 separate offsets would not stay in registers).
#pragma unroll
      for (int e = 0; e < 32; ++e) W[e] = 0;
      const uint8_t *q = slot;
#pragma unroll
      for (int k = 0; k < 64; ++k) {
        const int pos = kScanD[k], y = pos >> 3, x = pos & 7;
        const int code = *q;
        q += cols;
        if ((k & 7) == 7) asm volatile("" : "+v"(q));
        W[x * 4 + (y >> 1)] |= (uint32_t)(uint16_t)s_unmap[code] << ((y & 1) * 16);
      }
    }
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      const dupk16 d = __builtin_bit_cast(dupk16, W[e]) << __builtin_bit_cast(dupk16, shiftp[e]);
      V[e] = __builtin_bit_cast(dpk16, d);
      if (e != 0) rng.add(V[e]);
    }
  }
  dpk16 T[32];   // T[y*4 + i] = columns (2i, 2i+1) of row y after both passes
  if (__builtin_expect(packed_wht_exact(rng, V[0]), 1)) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      iwht8_pk(V[j], V[4 + j], V[8 + j], V[12 + j], V[16 + j], V[20 + j], V[24 + j], V[28 + j]);
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        T[y * 4 + i] = __builtin_bit_cast(
            dpk16, __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, V[(2 * i + 1) * 4 + (y >> 1)]),
                                         __builtin_bit_cast(uint32_t, V[(2 * i) * 4 + (y >> 1)]),
                                         (y & 1) ? 0x07060302u : 0x05040100u));
#pragma unroll
    for (int i = 0; i < 4; ++i)
      iwht8_pk(T[i], T[4 + i], T[8 + i], T[12 + i], T[16 + i], T[20 + i], T[24 + i], T[28 + i]);
  } else {
    // Scalar int32 path, one row / two columns at a time.
    uint32_t P[32];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      int r[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const uint32_t w = __builtin_bit_cast(uint32_t, V[x * 4 + (y >> 1)]);
        r[x] = (int)(int16_t)(uint16_t)(w >> ((y & 1) * 16));
      }
      iwht8(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
#pragma unroll
      for (int x = 0; x < 8; x += 2)
        P[y * 4 + x / 2] = ((uint32_t)r[x] & 0xffffu) | ((uint32_t)r[x + 1] << 16);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int ca[8], cb[8];
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        ca[y] = (int)(int16_t)(uint16_t)(P[y * 4 + i] & 0xffffu);
        cb[y] = (int)(int16_t)(uint16_t)(P[y * 4 + i] >> 16);
      }
      iwht8(ca[0], ca[1], ca[2], ca[3], ca[4], ca[5], ca[6], ca[7]);
      iwht8(cb[0], cb[1], cb[2], cb[3], cb[4], cb[5], cb[6], cb[7]);
#pragma unroll
      for (int y = 0; y < 8; ++y)
        T[y * 4 + i] = __builtin_bit_cast(dpk16, ((uint32_t)ca[y] & 0xffffu) | ((uint32_t)cb[y] << 16));
    }
  }
  uint32_t LQ[2][8];
  lowres_quads(lr0, lr8, LQ);
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    uint32_t sum[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t sel = 0x0c000c00u | (uint32_t)(y & 3) | ((uint32_t)(4 + (y & 3)) << 16);
      const dpk16 lo = __builtin_bit_cast(
          dpk16, __builtin_amdgcn_perm(LQ[y >> 2][2 * i + 1], LQ[y >> 2][2 * i], sel));
      sum[i] = __builtin_bit_cast(uint32_t, (dpk16)(T[y * 4 + i] + lo));
    }
    O[y * 2] = sat_pk_u8_hi(sat_pk_u8(sum[0]), sum[1]);
    O[y * 2 + 1] = sat_pk_u8_hi(sat_pk_u8(sum[2]), sum[3]);
  }
  (void)shift;
}

// One lane of a lane pair (lanes l and l + 32 of a wave: each half-wave then reads
// 32 adjacent symbol bytes of ONE plane per LDS instruction, free of bank
// conflicts): lane s transforms channels 2s and 2s+1 of tile u in block row v
// (packed int16 butterflies, see tile_plane), the pair swaps halves with one
// v_permlane32_swap per register pair, and lane s finishes pixel rows 4s..4s+3 --
// colour inverse on packed pairs (ycbcr.cpp:54-82), then two 16-byte stores per
// pixel row.  sym: the block row's symbols (channel c, scan index k, tile u at
// sym[(c*64 + k)*cols + u]), LDS or HBM; low: the frame's low-res planes.  Both
// lanes of a pair must be active (pair_tile / pair_half give the mapping).
// Item index -> (tile, half): 32 tiles per wave, lanes 0..31 half 0, lanes 32..63 half 1.
__device__ __forceinline__ int pair_tile(int it) { return (it >> 6) * 32 + (it & 31); }
__device__ __forceinline__ int pair_half(int it) { return (it >> 5) & 1; }

// The squared differences of the four bytes of a and b, added to acc: the bytes as packed int16
// pairs (even bytes, odd bytes), then v_dot2_i32_i16 of each difference with itself.
__device__ __forceinline__ uint32_t sse_word(uint32_t a, uint32_t b, uint32_t acc) {
  const uint32_t m = 0x00ff00ffu;
  const dpk16 e = __builtin_bit_cast(dpk16, a & m) - __builtin_bit_cast(dpk16, b & m);
  const dpk16 o = __builtin_bit_cast(dpk16, (a >> 8) & m) - __builtin_bit_cast(dpk16, (b >> 8) & m);
  int r = __builtin_amdgcn_sdot2(e, e, (int)acc, false);
  r = __builtin_amdgcn_sdot2(o, o, r, false);
  return (uint32_t)r;
}

// The planar float store form (TensDesc): the value of byte N of a packed word, one v_cvt_f32_ubyteN
// and one v_fma_f32; pairs of them rounded to nearest even into a dword of two float16 / bfloat16
// (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 -- never the round-toward-zero pack).  dtype is uniform
// across the launch: a scalar branch at the conversion, not a template parameter.
typedef const __attribute__((address_space(4))) TensDesc *TensK;   // in the kernel-argument segment
typedef float tens_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 tens_h2 __attribute__((ext_vector_type(2)));
typedef __bf16 tens_b2 __attribute__((ext_vector_type(2)));

template <int N>
__device__ __forceinline__ float tens_val(uint32_t w, float sc, float bi) {
  return __builtin_fmaf((float)((w >> (8 * N)) & 255u), sc, bi);
}
__device__ __forceinline__ uint32_t tens_pack(float a, float b, int dtype) {
  const tens_f2 v = {a, b};
  if (dtype == 1) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, tens_h2));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, tens_b2));
}
// Eight consecutive elements of one plane row from the packed bytes w0 (x = 0..3) and w1 (x = 4..7):
// one 16-byte store (float16 / bfloat16) or two (float32).  ALIGNED: dst is 16-byte aligned (the full
// decode of whole tiles).  Otherwise dst is only element-aligned (ragged widths, a window's rows) and
// elements [lo, hi) of the eight are real: all eight take the same 16-byte stores, which global memory
// accepts at any alignment; a tile cut by an edge stores its real elements one by one, from the same
// converted registers (dst itself may then lie in front of the buffer; nothing outside [lo, hi) is touched).
template <bool ALIGNED = true>
__device__ __forceinline__ void tens_store8(uint8_t *dst, uint32_t w0, uint32_t w1, float sc, float bi, int dtype,
                                            int lo = 0, int hi = 8) {
  const float v0 = tens_val<0>(w0, sc, bi), v1 = tens_val<1>(w0, sc, bi), v2 = tens_val<2>(w0, sc, bi),
              v3 = tens_val<3>(w0, sc, bi), v4 = tens_val<0>(w1, sc, bi), v5 = tens_val<1>(w1, sc, bi),
              v6 = tens_val<2>(w1, sc, bi), v7 = tens_val<3>(w1, sc, bi);
  const bool whole = ALIGNED || (lo == 0 && hi == 8);
  if (dtype == 0) {
    const float4 a = make_float4(v0, v1, v2, v3), b = make_float4(v4, v5, v6, v7);
    if (ALIGNED) {
      reinterpret_cast<float4 *>(dst)[0] = a;
      reinterpret_cast<float4 *>(dst)[1] = b;
    } else if (whole) {
      __builtin_memcpy(dst, &a, 16);
      __builtin_memcpy(dst + 16, &b, 16);
    } else {
      const float v[8] = {v0, v1, v2, v3, v4, v5, v6, v7};
#pragma unroll
      for (int x = 0; x < 8; ++x)
        if (x >= lo && x < hi) reinterpret_cast<float *>(dst)[x] = v[x];
    }
  } else {
    uint4 o;
    o.x = tens_pack(v0, v1, dtype); o.y = tens_pack(v2, v3, dtype);
    o.z = tens_pack(v4, v5, dtype); o.w = tens_pack(v6, v7, dtype);
    if (ALIGNED) {
      *reinterpret_cast<uint4 *>(dst) = o;
    } else if (whole) {
      __builtin_memcpy(dst, &o, 16);
    } else {
      const uint32_t p[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int x = 0; x < 8; ++x)
        if (x >= lo && x < hi) reinterpret_cast<uint16_t *>(dst)[x] = (uint16_t)(p[x >> 1] >> (16 * (x & 1)));
    }
  }
}
// The lane's packed bytes of one half row (q0..q3: channels 0..3, x = 4h..4h+3) as the channels the
// picture has: the colour inverse of transform_store_pair (ycbcr.cpp:54-82, two pixels per packed
// operation), its saturated pairs merged per channel instead of interleaved per pixel.
__device__ __forceinline__ void tens_planes(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, int ycbcr,
                                            uint32_t &p0, uint32_t &p1, uint32_t &p2, uint32_t &p3) {
  if (ycbcr) {
    uint32_t rs[2], gs[2], bs[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint32_t sel = k ? 0x0c030c02u : 0x0c010c00u;
      const dpk16 yy = __builtin_bit_cast(dpk16, __builtin_amdgcn_perm(0u, q0, sel));
      const dpk16 cbq = __builtin_bit_cast(dpk16, __builtin_amdgcn_perm(0u, q1, sel));
      const dpk16 crq = __builtin_bit_cast(dpk16, __builtin_amdgcn_perm(0u, q2, sel));
      const dpk16 c255 = {255, 255}, c254 = {254, 254}, one = {1, 1};
      const dpk16 gg = yy - ((cbq + crq - c254) >> one);
      const dpk16 g255 = gg - c255;
      rs[k] = sat_pk_u8(pk_mad2(crq, g255));
      gs[k] = sat_pk_u8(__builtin_bit_cast(uint32_t, gg));
      bs[k] = sat_pk_u8(pk_mad2(cbq, g255));
    }
    p0 = __builtin_amdgcn_perm(rs[1], rs[0], 0x05040100u);
    p1 = __builtin_amdgcn_perm(gs[1], gs[0], 0x05040100u);
    p2 = __builtin_amdgcn_perm(bs[1], bs[0], 0x05040100u);
  } else {
    p0 = q0; p1 = q1; p2 = q2;
  }
  p3 = q3;
}
// The pitched destination (DstDesc) in the kernel-argument segment.  dst_at_use: the pointer made
// opaque where the stores begin, so that the loads of the pitch and the stride cannot be moved up in
// front of the transform and stay live across it.
typedef const __attribute__((address_space(4))) DstDesc *DstK;
__device__ __forceinline__ DstK dst_at_use(DstK pd) {
  asm volatile("" : "+s"(pd));
  return pd;
}
// Frame f's origin pixel in the destination (f is uniform: scalar loads).
__device__ __forceinline__ uint8_t *dst_frame(uint8_t *out, DstK pd, int f) {
  const int32_t *org = pd->org;
  return out + (size_t)f * pd->frame_pitch + (size_t)org[2 * f + 1] * pd->row_pitch +
         (size_t)org[2 * f] * (size_t)pd->pixel_stride;
}
// The wanted planes (PlaneDesc) in the kernel-argument segment.  planes_at_use: the pointer made
// opaque where the stores begin, so that the mask is read again there and is not live across the transform.
typedef const __attribute__((address_space(4))) PlaneDesc *PlaneK;
__device__ __forceinline__ PlaneK planes_at_use(PlaneK pc) {
  asm volatile("" : "+s"(pc));
  return pc;
}
// FULL4: four channels, whole tiles only (W and H multiples of 8) -- the ragged-edge
// stores and the channel-count tests are compiled out.
// SSE (k_sse, the encoder's distortion probe): nothing is stored -- the lane's four pixel rows are
// compared with the source picture instead (src: the frame, sstride bytes per pixel of which the
// first C count; FULL4: packed RGBA, two 16-byte loads per pixel row) and the sum of the squared
// differences over the real pixels is returned (at most 4 * 8 * 4 * 255^2 < 2^24).
// TENS (the tensor forms of the row kernels): the planar float output instead of the interleaved
// bytes -- img is frame f's [co][H][W] elements, td the descriptor in the kernel-argument segment,
// read here at its use.  The lane converts its four pixel rows from the per-channel packed bytes
// (ch0..ch3, or the saturated r / g / b pairs behind the colour inverse) and never interleaves them:
// FULL4 eight consecutive elements per channel and pixel row (adjacent lanes adjacent tiles: a
// wavefront's stores are contiguous along the row), 16-byte aligned; otherwise the same stores at
// element alignment for whole tiles and element stores for the ragged right edge (tens_store8), rows
// masked to H and channels to co.
// Channels from co on are neither converted nor stored.
// PITCH (the pitched forms): the same pixel words at img + (8 v + y) * row_pitch + 8 u * pixel_stride,
// img frame f's origin pixel (dst_frame), pd the descriptor in the kernel-argument segment, read at
// the stores.  Which store, per tile row and from the address itself: 4-byte pixels of four channels --
// a whole tile row at a 16-byte aligned address the two 16-byte stores, otherwise a dword per real
// pixel (the host checks make every pixel 4-byte aligned); everything else the C channel bytes of
// every real pixel.  No store covers a byte that is not a channel byte of a pixel of the picture.
// PLANES (the planes forms): the stream's own channel planes -- img is frame f's [P][H][W] bytes, pl
// the descriptor in the kernel-argument segment.  Of the lane's two channels, step cc of the transform
// (channel cc for the lower half of the wavefront, 2 + cc for the upper) runs only where the mask wants
// one of the two: a uniform branch, and tile_plane is not run for a step nobody asked for.  Behind the
// swap the lane holds its four pixel rows of every channel as packed bytes (ch0..ch3), byte k of a
// word x = 4h + k: a wanted plane's tile row is stored as it is -- no colour inverse, no interleave --,
// one 8-byte store where the tile is whole and the address a multiple of 8 (FULL4: always), else a
// byte per real pixel; rows masked to H.
template <int COLS, bool FULL4 = false, bool SSE = false, bool TENS = false, bool PITCH = false, bool PLANES = false>
__device__ __forceinline__ uint32_t transform_store_pair(const Geom &g, int cols_rt, const uint8_t *sym,
                                                     const uint8_t *low, const int16_t *s_unmap,
                                                     const uint8_t *s_shift, const uint32_t *s_shiftp,
                                                     int ycbcr, int u, int s, int v, uint8_t *img,
                                                     const uint32_t *pre_lr = nullptr, bool store_ok = true,
                                                     bool touched_on = false, uint32_t touched = 0,
                                                     const uint8_t *src = nullptr, int sstride = 0,
                                                     TensK td = nullptr, DstK pd = nullptr, PlaneK pl = nullptr) {
  uint32_t sse = 0;
  const int cols = COLS > 0 ? COLS : cols_rt;
  const int C = FULL4 ? 4 : g.C;
  const int v2 = min(v + 1, g.rows - 1);
    const int u2 = min(u + 1, cols - 1);
    // (PLANES: which of the two steps are wanted -- uniform, a scalar load)
    uint32_t want_cc = 3u;
    if constexpr (PLANES) {
      const uint32_t m = pl->mask;
      want_cc = ((m | (m >> 2)) & 3u);
    }
    uint32_t QA[16], QB[16];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int c = 2 * s + cc;
      uint32_t O[16];
      if ((FULL4 || c < C) && (!PLANES || ((want_cc >> cc) & 1u))) {
        const uint8_t *m = low + (size_t)c * g.rows * cols;
        const int chroma = (ycbcr && (c == 1 || c == 2)) ? 1 : 0;  // decoder.cpp:376
        uint32_t lr0, lr8;
        if (pre_lr) {   // (inlined: a compile-time choice)
          lr0 = pre_lr[2 * cc]; lr8 = pre_lr[2 * cc + 1];
        } else {
          lr0 = (uint32_t)m[(size_t)v * cols + u] | ((uint32_t)m[(size_t)v * cols + u2] << 8);
          lr8 = (uint32_t)m[(size_t)v2 * cols + u] | ((uint32_t)m[(size_t)v2 * cols + u2] << 8);
        }
        tile_plane<COLS>(sym + (size_t)c * 64 * cols + u, cols, s_unmap, s_shift + chroma * 64,
                         s_shiftp + chroma * 32, lr0, lr8, O, COLS != 0 ? s_shiftp + 64 + 2 * chroma : nullptr);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) O[i] = 0;
      }
      if (cc == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) QA[i] = O[i];
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) QB[i] = O[i];
      }
    }
    // Swap halves between lane l and lane l + 32: one v_permlane32_swap per register
    // pair hands the upper lanes the partner's rows 4..7 of channels 0/1 and the
    // lower lanes the partner's rows 0..3 of channels 2/3 -- afterwards either half
    // holds its four pixel rows of all four channels, no selects.
    uint32_t ch0[8], ch1[8], ch2[8], ch3[8];   // [r*2+h]: pixel row 4s+r, x = 4h..4h+3
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const auto ra = __builtin_amdgcn_permlane32_swap(QA[i], QA[8 + i], false, false);
      const auto rb = __builtin_amdgcn_permlane32_swap(QB[i], QB[8 + i], false, false);
      ch0[i] = ra[0]; ch2[i] = ra[1];
      ch1[i] = rb[0]; ch3[i] = rb[1];
    }
    const int bw = FULL4 ? 8 : min(8, g.W - 8 * u);
    const int bh = FULL4 ? 8 : min(8, g.H - 8 * v);
    if (touched_on) {
      // (k_dec_row_fused's touch loads for the next row: issued before the gather, long landed --
      // their registers are given back here, in front of the pixel stores, so that nothing waits
      // for a store.)
      __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
      asm volatile("" :: "v"(touched));
    }
    // (PITCH: the pitch and the stride, read once here -- behind the transform, for the four rows)
    size_t row_pitch = 0;
    int ps = 0;
    if constexpr (PITCH) {
      const DstK pk = dst_at_use(pd);
      row_pitch = pk->row_pitch; ps = pk->pixel_stride;
    }
    // (PLANES: the mask, read again here -- behind the transform, for the four rows)
    uint32_t pmask = 0;
    if constexpr (PLANES) pmask = planes_at_use(pl)->mask;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int y = 4 * s + rr;
      if constexpr (PLANES) {
        if (store_ok && (FULL4 || y < bh)) {
          size_t e = (size_t)(8 * v + y) * g.W + (size_t)(8 * u);   // the tile row in the next wanted plane
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if ((pmask >> c) & 1u) {   // (uniform; the host has refused a bit at or above C)
              const uint32_t lo = c == 0 ? ch0[rr * 2] : c == 1 ? ch1[rr * 2] : c == 2 ? ch2[rr * 2] : ch3[rr * 2];
              const uint32_t hi = c == 0 ? ch0[rr * 2 + 1] : c == 1 ? ch1[rr * 2 + 1] : c == 2 ? ch2[rr * 2 + 1] : ch3[rr * 2 + 1];
              uint8_t *dst = img + e;
              if (FULL4 || (bw == 8 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0)) {
                uint2 o;
                o.x = lo; o.y = hi;
                *reinterpret_cast<uint2 *>(dst) = o;
              } else {
#pragma unroll
                for (int x = 0; x < 8; ++x)
                  if (x < bw) dst[x] = (uint8_t)((x < 4 ? lo : hi) >> (8 * (x & 3)));
              }
              e += (size_t)g.H * g.W;
            }
          }
        }
      } else if constexpr (TENS) {
        uint32_t pc[4][2];   // [channel][h]: the bytes of x = 4h..4h+3
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t q0 = ch0[rr * 2 + h], q1 = ch1[rr * 2 + h], q2 = ch2[rr * 2 + h], q3 = ch3[rr * 2 + h];
          tens_planes(q0, q1, q2, q3, ycbcr, pc[0][h], pc[1][h], pc[2][h], pc[3][h]);
        }
        if (store_ok && (FULL4 || y < bh)) {
          const int dtype = td->dtype, co = td->co;
          const size_t es = (size_t)tens_elem_size(dtype);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (c < co) {
              const float sc = td->scale[c], bi = td->bias[c];
              const size_t e = ((size_t)c * g.H + (size_t)(8 * v + y)) * g.W + (size_t)(8 * u);
              if (FULL4) tens_store8(img + e * es, pc[c][0], pc[c][1], sc, bi, dtype);
              else tens_store8<false>(img + e * es, pc[c][0], pc[c][1], sc, bi, dtype, 0, bw);
            }
          }
        }
      } else {
      uint32_t px[8];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t q0 = ch0[rr * 2 + h], q1 = ch1[rr * 2 + h], q2 = ch2[rr * 2 + h], q3 = ch3[rr * 2 + h];
        if (ycbcr) {  // ycbcr.cpp:54-82, two pixels per packed op
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const uint32_t sel = k ? 0x0c030c02u : 0x0c010c00u;
            const dpk16 yy = __builtin_bit_cast(dpk16, __builtin_amdgcn_perm(0u, q0, sel));
            const dpk16 cbq = __builtin_bit_cast(dpk16, __builtin_amdgcn_perm(0u, q1, sel));
            const dpk16 crq = __builtin_bit_cast(dpk16, __builtin_amdgcn_perm(0u, q2, sel));
            const dpk16 c255 = {255, 255}, c254 = {254, 254}, one = {1, 1};
            // cbv = 2 cb - 255, crv = 2 cr - 255;  (cbv + crv + 2) >> 2 == (cb + cr - 254) >> 1 exactly.
            const dpk16 gg = yy - ((cbq + crq - c254) >> one);
            // r = g + crv, b = g + cbv as ONE multiply-add each on top of g - 255 (v_pk_mad_i16:
            // three packed operations for the pair instead of six; everything stays far inside int16).
            const dpk16 g255 = gg - c255;
            const uint32_t rs = sat_pk_u8(pk_mad2(crq, g255));
            const uint32_t gs = sat_pk_u8(__builtin_bit_cast(uint32_t, gg));
            const uint32_t bs = sat_pk_u8(pk_mad2(cbq, g255));
            const uint32_t rg = __builtin_amdgcn_perm(gs, rs, 0x05010400u);            // r0 g0 r1 g1
            const uint32_t ba = __builtin_amdgcn_perm(q3, bs, k ? 0x07010600u : 0x05010400u);  // b0 a0 b1 a1
            px[4 * h + 2 * k] = __builtin_amdgcn_perm(ba, rg, 0x05040100u);
            px[4 * h + 2 * k + 1] = __builtin_amdgcn_perm(ba, rg, 0x07060302u);
          }
        } else {
          const uint32_t t0 = __builtin_amdgcn_perm(q1, q0, 0x05010400u), t1 = __builtin_amdgcn_perm(q1, q0, 0x07030602u);
          const uint32_t w0 = __builtin_amdgcn_perm(q3, q2, 0x05010400u), w1 = __builtin_amdgcn_perm(q3, q2, 0x07030602u);
          px[4 * h + 0] = __builtin_amdgcn_perm(w0, t0, 0x05040100u);
          px[4 * h + 1] = __builtin_amdgcn_perm(w0, t0, 0x07060302u);
          px[4 * h + 2] = __builtin_amdgcn_perm(w1, t1, 0x05040100u);
          px[4 * h + 3] = __builtin_amdgcn_perm(w1, t1, 0x07060302u);
        }
      }
      if constexpr (SSE) {
        if (FULL4 || y < bh) {
          if (FULL4) {
            const uint4 *sp = reinterpret_cast<const uint4 *>(src + ((size_t)(8 * v + y) * g.W + 8 * u) * 4);
            const uint4 a0 = sp[0], a1 = sp[1];
            sse = sse_word(px[0], a0.x, sse); sse = sse_word(px[1], a0.y, sse);
            sse = sse_word(px[2], a0.z, sse); sse = sse_word(px[3], a0.w, sse);
            sse = sse_word(px[4], a1.x, sse); sse = sse_word(px[5], a1.y, sse);
            sse = sse_word(px[6], a1.z, sse); sse = sse_word(px[7], a1.w, sse);
          } else {
            const uint8_t *sp = src + ((size_t)(8 * v + y) * g.W + 8 * u) * sstride;
#pragma unroll
            for (int x = 0; x < 8; ++x)
              if (x < bw)
                for (int c = 0; c < C; ++c) {
                  const int d = (int)((px[x] >> (8 * c)) & 255u) - (int)sp[x * sstride + c];
                  sse += (uint32_t)(d * d);
                }
          }
        }
      } else if constexpr (PITCH) {
        if (store_ok && (FULL4 || y < bh)) {
          uint8_t *dst = img + (size_t)(8 * v + y) * row_pitch + (size_t)(8 * u) * (size_t)ps;
          if (C == 4 && ps == 4) {
            if ((FULL4 || bw == 8) && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
              uint4 o0, o1;
              o0.x = px[0]; o0.y = px[1]; o0.z = px[2]; o0.w = px[3];
              o1.x = px[4]; o1.y = px[5]; o1.z = px[6]; o1.w = px[7];
              reinterpret_cast<uint4 *>(dst)[0] = o0;
              reinterpret_cast<uint4 *>(dst)[1] = o1;
            } else {
#pragma unroll
              for (int x = 0; x < 8; ++x)
                if (x < bw) reinterpret_cast<uint32_t *>(dst)[x] = px[x];
            }
          } else {
#pragma unroll
            for (int x = 0; x < 8; ++x)
              if (x < bw)
                for (int c = 0; c < C; ++c) dst[(size_t)x * ps + c] = (uint8_t)(px[x] >> (8 * c));
          }
        }
      } else
      if (store_ok && (FULL4 || y < bh)) {
        uint8_t *dst = img + ((size_t)(8 * v + y) * g.W + 8 * u) * C;
        if (FULL4 || (C == 4 && bw == 8)) {
          uint4 o0, o1;
          o0.x = px[0]; o0.y = px[1]; o0.z = px[2]; o0.w = px[3];
          o1.x = px[4]; o1.y = px[5]; o1.z = px[6]; o1.w = px[7];
          reinterpret_cast<uint4 *>(dst)[0] = o0;
          reinterpret_cast<uint4 *>(dst)[1] = o1;
        } else {
#pragma unroll
          for (int x = 0; x < 8; ++x)
            if (x < bw)
              for (int c = 0; c < C; ++c) dst[x * C + c] = (uint8_t)(px[x] >> (8 * c));
        }
      }
      }   // (!TENS)
    }
    return sse;
}

// tile_plane's identity test, by one wavefront (l = 0..63).  n = the largest code with
// fmap[i] == i for all i <= n (mapper.h:33-35: a code unmaps to itself there);
// B = the largest power of two <= n, lowered until B << (largest shift of group H:
// rows 2..7 of columns 1..7) <= 2048 (inside both range conditions of the packed
// transform, packed_wht_exact).  dst[2 * chroma + {0, 1}]: (B, B), then the mask of the
// bits that a sum code + B outside [0, 2B) sets.  No usable range: the test always fails.
__device__ __forceinline__ void identity_test_words(const DecFrame *df, int l, uint32_t *dst) {
  const unsigned long long ne = __ballot(df->fmap[l] != l), ne2 = __ballot(df->fmap[64 + l] != 64 + l);
  const int n = ne ? __ffsll((long long)ne) - 2 : (ne2 ? 62 + __ffsll((long long)ne2) : 127);
  if (l < 2) {
    int smax = 0;
    for (int y = 2; y < 8; ++y)
      for (int x = 1; x < 8; ++x) smax = max(smax, (int)df->shift[l][y * 8 + x]);
    int B = 0;
    if (n >= 1) {
      B = 1 << (31 - __clz(n));
      while (B && ((long long)B << smax) > 2048) B >>= 1;
    }
    const uint32_t b16 = B ? (uint32_t)B : 0x4000u, m16 = B ? (uint32_t)(0xffffu & ~(2u * B - 1u)) : 0xffffu;
    dst[2 * l] = b16 | (b16 << 16);
    dst[2 * l + 1] = m16 | (m16 << 16);
  }
}

// k_tile_inv: the transform of the unfused path (rows too wide for LDS): the
// symbols come from HBM (ws.fres_sym, written by k_dec_huff); two lanes per tile,
// 128 tiles per workgroup.
// FAST: four channels, whole tiles (tile_plane's identity-range gather, no ragged edges).
template <bool FAST>
__global__ __launch_bounds__(256) void k_tile_inv(Geom g, DecWs ws, uint8_t *out_frames, int v0) {
#include "dec_body_tile_inv.inc"
  transform_store_pair<(FAST ? -1 : 0), FAST>(g, g.cols, ws.fres_sym + (size_t)f * ws.fres_stride + (size_t)v * g.row_block,
                          ws.low + (size_t)f * ws.plane_stride, s_unmap, &s_shift[0][0], s_shiftp,
                          df->ycbcr, pair_tile(it), pair_half(it), v,
                          out_frames + (size_t)f * ((size_t)g.W * g.H * g.C));
}

// k_tile_inv_t: k_tile_inv in its tensor form (TensDesc): frame f's [co][H][W] elements at
// out_frames + f * co * H * W elements.  The arguments in one struct, so that the descriptor is
// read from the kernel-argument segment where the stores use it.
struct TileArgsT {
  Geom g;
  DecWs ws;
  uint8_t *out_frames;
  int v0;
  TensDesc t;
};
template <bool FAST>
__global__ __launch_bounds__(256) void k_tile_inv_t(TileArgsT a) {
  const Geom &g = a.g;
  const DecWs &ws = a.ws;
  const int v0 = a.v0;
  const TensK td = &((const __attribute__((address_space(4))) TileArgsT *)__builtin_amdgcn_kernarg_segment_ptr())->t;
#include "dec_body_tile_inv.inc"
  const size_t frame_bytes = (size_t)g.W * g.H * (size_t)(td->co * tens_elem_size(td->dtype));
  transform_store_pair<(FAST ? -1 : 0), FAST, false, true>(
      g, g.cols, ws.fres_sym + (size_t)f * ws.fres_stride + (size_t)v * g.row_block,
      ws.low + (size_t)f * ws.plane_stride, s_unmap, &s_shift[0][0], s_shiftp, df->ycbcr, pair_tile(it),
      pair_half(it), v, a.out_frames + (size_t)f * frame_bytes, nullptr, true, false, 0, nullptr, 0, td);
}

// k_tile_inv_p: k_tile_inv in its pitched form (DstDesc): frame f's picture at its origin in the
// destination.  The arguments in one struct, as in k_tile_inv_t.
struct TileArgsP {
  Geom g;
  DecWs ws;
  uint8_t *out_frames;
  int v0;
  DstDesc d;
};
template <bool FAST>
__global__ __launch_bounds__(256) void k_tile_inv_p(TileArgsP a) {
  const Geom &g = a.g;
  const DecWs &ws = a.ws;
  const int v0 = a.v0;
  const DstK pd = &((const __attribute__((address_space(4))) TileArgsP *)__builtin_amdgcn_kernarg_segment_ptr())->d;
#include "dec_body_tile_inv.inc"
  transform_store_pair<(FAST ? -1 : 0), FAST, false, false, true>(
      g, g.cols, ws.fres_sym + (size_t)f * ws.fres_stride + (size_t)v * g.row_block,
      ws.low + (size_t)f * ws.plane_stride, s_unmap, &s_shift[0][0], s_shiftp, df->ycbcr, pair_tile(it),
      pair_half(it), v, dst_frame(a.out_frames, pd, f), nullptr, true, false, 0, nullptr, 0, nullptr, pd);
}

// k_tile_inv_c: k_tile_inv in its planes form (PlaneDesc): frame f's [P][H][W] bytes at
// out_frames + f * P * H * W.  The arguments in one struct, as in k_tile_inv_t.
struct TileArgsC {
  Geom g;
  DecWs ws;
  uint8_t *out_frames;
  int v0;
  PlaneDesc c;
};
template <bool FAST>
__global__ __launch_bounds__(256) void k_tile_inv_c(TileArgsC a) {
  const Geom &g = a.g;
  const DecWs &ws = a.ws;
  const int v0 = a.v0;
  const PlaneK pc = &((const __attribute__((address_space(4))) TileArgsC *)__builtin_amdgcn_kernarg_segment_ptr())->c;
#include "dec_body_tile_inv.inc"
  const size_t frame_bytes = (size_t)g.W * g.H * (size_t)plane_count(pc->mask);
  transform_store_pair<(FAST ? -1 : 0), FAST, false, false, false, true>(
      g, g.cols, ws.fres_sym + (size_t)f * ws.fres_stride + (size_t)v * g.row_block,
      ws.low + (size_t)f * ws.plane_stride, s_unmap, &s_shift[0][0], s_shiftp, df->ycbcr, pair_tile(it),
      pair_half(it), v, a.out_frames + (size_t)f * frame_bytes, nullptr, true, false, 0, nullptr, 0, nullptr, nullptr, pc);
}

// ---------------------------------------------------------------------------
// k_sse: the encoder's distortion probe (himg_hip_encode_sse_device).  k_tile_inv's transform on
// the ENCODER's symbol plane (the same [rows][C][64][cols] layout) and its reconstructed low-res
// plane, with the decode-side tables of the frame's quality from the context's per-quality table
// instead of a parsed stream's -- and instead of storing the pixels it compares them with the
// source and adds the squared differences up.  No entropy coder ran in either direction.
// Two lanes per tile, 128 tiles per workgroup.  FAST: packed RGBA, whole tiles.
// The sum: below 2^24 per lane, below 2^30 per wavefront (32 bits), 64 bits across the
// workgroup's wavefronts, then ONE 64-bit vector atomic add per workgroup: integer adds, so the
// result does not depend on their order.
// ---------------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(256) void k_sse(Geom g, const uint8_t *frames, const uint8_t *fres_sym, size_t fres_stride,
                                             const uint8_t *rec, size_t plane_stride, const SseTab *tabs,
                                             const int32_t *quality, unsigned long long *sse) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[kRowTabWords];
  __shared__ unsigned long long s_part[4];
  const int v = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
  // (the frame index is uniform: its quality is one scalar load)
  const int q = __builtin_amdgcn_readfirstlane(
      ((const __attribute__((address_space(4))) int32_t *)(uintptr_t)quality)[f]);
  if (tid < kRowTabWords / 4) reinterpret_cast<uint4 *>(s_tab)[tid] = reinterpret_cast<const uint4 *>(tabs[q].w)[tid];
  __syncthreads();
  const int16_t *s_unmap = reinterpret_cast<const int16_t *>(s_tab);
  const uint8_t *s_shift = reinterpret_cast<const uint8_t *>(s_tab + 128);
  const uint32_t *s_shiftp = s_tab + 160;
  const int it = blockIdx.x * 256 + tid;   // (tile, half): both lanes of a pair are in or out
  uint32_t acc = 0;
  if (pair_tile(it) < g.cols)
    acc = transform_store_pair<(FAST ? -1 : 0), FAST, true>(
        g, g.cols, fres_sym + (size_t)f * fres_stride + (size_t)v * g.row_block, rec + (size_t)f * plane_stride,
        s_unmap, s_shift, s_shiftp, g.ycbcr, pair_tile(it), pair_half(it), v, nullptr, nullptr, true, false, 0,
        frames + (size_t)f * (size_t)g.frame_bytes, g.stride);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if ((tid & 63) == 0) s_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long t = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    if (t) __hip_atomic_fetch_add(sse + f, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// COLS > 0 fixes the tile count per block row at compile time (512 = 4096-pixel
// rows; COLS < 0: any width of four-channel whole tiles, run-time count, the same transform paths): the 64 symbol slots of a tile are then at immediate LDS offsets instead
// of 64 live address registers, which is what keeps the transform phase from
// spilling.
// A workgroup takes `rpw` consecutive block rows: narrow rows leave most of the 1024
// lanes without a tile in the transform (two lanes per tile: 480 lanes at 1920
// pixels), so as many rows as fit the LDS -- and the lanes -- are entropy-decoded one
// after the other (each by all 1024 lanes) and then transformed together.
// TENS: the planar float output (transform_store_pair's tensor form); out_frames is then the
// [batch][co][H][W] buffer and td the descriptor in the kernel-argument segment.
// PITCH: the pitched output (transform_store_pair's pitched form); out_frames is then the first
// destination picture and pd the descriptor in the kernel-argument segment.
// PYR: the picture pyramid (PyrDesc, pm in the kernel-argument segment); out_frames is level 0, which
// the loop above stores when it is wanted; a second loop over the rows' tiles then computes the wanted
// ones of the 1/2- and 1/4-scale levels from the same symbols in LDS (pyr_tile_part: k_dec_scaled's
// tile arithmetic at stride cols, channel stride 64 cols).
// PLANES: the stream's own planes (transform_store_pair's planes form); out_frames is then the
// [batch][P][H][W] buffer and pc the descriptor in the kernel-argument segment.
template <int PART>
__device__ __forceinline__ void pyr_tile_part(const Geom &g, int sstride, int cstride, const uint8_t *sym,
                                              const uint8_t *low, const int16_t *s_unmap, const uint8_t *s_shift,
                                              int ycbcr, int u, int v, int f, uint8_t *level);   // (behind scaled_tile_rows)
typedef const __attribute__((address_space(4))) PyrDesc *PyrK;
template <int COLS, bool TENS = false, bool PITCH = false, bool PYR = false, bool PLANES = false>
__device__ __forceinline__ void dec_row_fused_body(const Geom &g, const DecWs &ws, const uint8_t *packed,
                                                   size_t in_stride, const uint32_t *sizes,
                                                   uint8_t *out_frames, int r0, int r1, int rpw,
                                                   const int bx, const int f, const int gx, const int gy,
                                                   const uint32_t next_lin, const bool again, const bool same_tables,
                                                   TensK td = nullptr, DstK pd = nullptr, PyrK pm = nullptr,
                                                   PlaneK pc = nullptr) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if (COLS == 512) rpw = 1;   // 4096-pixel rows: one row fills the lanes and the LDS (known at compile time)
  const FusedLayout L = fused_layout(g.row_block, rpw);
  const uint32_t rb16 = ((uint32_t)g.row_block + 15u) & ~15u;   // one row's symbols
  uint8_t *sym0 = smem + L.sym;
  LdsTables &T = *reinterpret_cast<LdsTables *>(smem + L.tab);
  StreamShared *sh = reinterpret_cast<StreamShared *>(smem + L.sh);
  int16_t *s_unmap = reinterpret_cast<int16_t *>(smem + L.unmap);
  uint8_t *s_shift = smem + L.shift;
  uint32_t *s_shiftp = reinterpret_cast<uint32_t *>(smem + L.shiftp);

  // (opaque per row: what depends on the lane alone would otherwise be computed once in front of
  // the persistent loop and stay in registers across the whole body)
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));
  __builtin_assume(tid_ >= 0 && tid_ < kDecThreads);   // (the range the compiler knew of threadIdx.x)
  const int tid = tid_;
  const long long c_in = clock64();
  DecFrame *df = ws.frames + f;
  const uint8_t *low = ws.low + (size_t)f * ws.plane_stride;
  // 4096-pixel rows: one row per workgroup, every lane knows its tile from the start.
  // Everything the row needs from global memory is requested HERE, in front of the
  // first barrier -- the frame's verdict, k_row_count's lane record, the row index,
  // the low-res corners of the lane's two planes, the tables -- so that the round
  // trips overlap instead of following each other (each is 1-2 us of a 43 us row).
  PreLane pl = {};
  uint32_t pre_lr[4] = {0, 0, 0, 0}, pre_off0 = 0, pre_len0 = 0;
  if constexpr (COLS == 512) {
    const size_t ri = (size_t)f * g.rows + (size_t)(r0 + bx);
    const uint32_t *ps = ws.lane_start + ri * kDecThreads, *po = ws.lane_off + ri * (kDecThreads + kRecHdr);
    pl.start = ps[tid]; pl.off = po[tid]; pl.nxt = po[tid + 1];
    pl.nstart = tid + 1 < kDecThreads ? ps[tid + 1] : ~0u;
    pl.tot = po[kDecThreads]; pl.endrel = po[kDecThreads + 1]; pl.valid = po[kDecThreads + 2]; pl.rounds = po[kDecThreads + 3];
    pre_off0 = ws.row_off[ri]; pre_len0 = ws.row_len[ri];
    const int u = pair_tile(tid), hs = pair_half(tid), v = r0 + bx;
    const int u2 = min(u + 1, COLS - 1), v2 = min(v + 1, g.rows - 1);
    // (32-bit offsets from the frame's plane: a low-res plane set is C * rows * cols bytes)
    const uint32_t pstride = (uint32_t)g.rows * COLS, o1 = (uint32_t)v * COLS, o2 = (uint32_t)v2 * COLS;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const uint32_t m = (uint32_t)(2 * hs + cc) * pstride;
      pre_lr[2 * cc] = (uint32_t)low[m + o1 + u] | ((uint32_t)low[m + o1 + u2] << 8);
      pre_lr[2 * cc + 1] = (uint32_t)low[m + o2 + u] | ((uint32_t)low[m + o2 + u2] << 8);
    }
  }
  // The frame's verdict: ONE read for the workgroup (other workgroups flag the frame
  // concurrently).  4096-pixel rows: requested here, stored with the tables below -- a
  // store right here would make wave 0 wait for every load above before it requests
  // its share of the tables, two round trips in front of the first barrier.
  uint32_t st0 = 0;
  if (tid == 0) st0 = df->status;
  if constexpr (COLS != 512) {
    // A persistent workgroup's next row: the row before may have ended on a verdict read from the
    // LDS with no barrier behind the read (sh->flag of a failed frame just below, sh->err of a
    // failed row) -- a slow wavefront that has not read it yet must not meet this row's flag, or
    // it stays in a row the others have left and its barriers pair with the wrong ones.  This is
    // also the barrier in front of the LDS writes below (4096-pixel rows have it there).
    if (again) __syncthreads();
    if (tid == 0) sh->flag = st0;
    __syncthreads();
    if (sh->flag) return;
  }
  const uint8_t *p = packed + (size_t)f * in_stride;
  // The decode tables: the loads first (one group-table and one sub-table quad-word
  // per lane, a tree node for the first 522 -- every slot of the workspace, so that the
  // node count need not be known), then the clear of the symbol area below while they
  // are in flight, then the stores.
  static_assert((1 << kLutBits) / 2 == kDecThreads && kSubEntries / 2 <= kDecThreads && kMaxNodes + 1 <= kDecThreads,
                "one table element per lane");
  // (A persistent workgroup whose last row was of the same frame still holds them.)
  const bool ld_tab = !(COLS == 512 && same_tables);
  uint4 t_grp = make_uint4(0, 0, 0, 0), t_sub = t_grp, t_row = t_grp;
  uint32_t t_nd = 0;
  static_assert(kRowTabWords / 4 <= 64, "one wavefront copies them");
  if (ld_tab) {
    t_grp = reinterpret_cast<const uint4 *>(ws.grp + ((size_t)f * 2 + 1) * (1u << kLutBits))[tid];
    if (tid < kSubEntries / 2) t_sub = reinterpret_cast<const uint4 *>(ws.sub + ((size_t)f * 2 + 1) * kSubEntries)[tid];
    if (tid < kMaxNodes + 1) t_nd = (ws.nodes + ((size_t)f * 2 + 1) * (kMaxNodes + 1))[tid];
    // The transform's tables: one 16-byte word per lane of wave 0 from the frame's copy (k_dec_parse).
    if (tid < kRowTabWords / 4) t_row = reinterpret_cast<const uint4 *>(df->row_tabs)[tid];
  }
  const GrpTables tb = tables_of(&T);
  const int rb = r0 + bx * rpw;
  const int nr = COLS == 512 ? 1 : min(rpw, r1 - rb);
  // A persistent workgroup's next row: the loads above are in flight while the slowest wavefront
  // still transforms the row before; nothing of the LDS is written before it is done.
  // (Other widths: that barrier stands in front of the flag store above.)
  if (COLS == 512 && again) __syncthreads();
  {
    uint4 z;
    z.x = z.y = z.z = z.w = 0;
    const int n16 = (int)(rb16 >> 4) * nr;
    for (int k = tid; k < n16; k += kDecThreads) reinterpret_cast<uint4 *>(sym0)[k] = z;
  }
  if (ld_tab) {
    reinterpret_cast<uint4 *>(T.grp)[tid] = t_grp;
    if (tid < kRowTabWords / 4) reinterpret_cast<uint4 *>(smem + L.unmap)[tid] = t_row;   // unmap, shift, shiftp: contiguous
    if (tid < kSubEntries / 2) reinterpret_cast<uint4 *>(T.grp + (1 << kLutBits))[tid] = t_sub;
    if (tid < kMaxNodes + 1) T.nd[tid] = t_nd;
  }
  if constexpr (COLS == 512) {
    if (tid == 0) { sh->flag = st0; sh->err = 0; sh->endbit = ~0ull; }   // (decode_stream<.., PRIMED>)
  }
  __syncthreads();
  if constexpr (COLS == 512) {
    if (sh->flag) return;   // (uniform: one read, in front of the barrier above)
  }

  auto decode_row = [&](int i) {
    const int r = rb + i;
    if (tid == 0) {
      uint32_t *st = ws.stats + ((size_t)f * (g.rows + 1) + r + 1) * 8;
      st[2] = 0; st[3] = 0;   // atomicMax targets, see the end of the kernel
    }
    if constexpr (COLS == 512) {
      uint32_t *st = ws.stats + ((size_t)f * (g.rows + 1) + r + 1) * 8;
      const int rc = decode_row_recorded(p, sizes[f], pre_off0, pre_len0, (uint32_t)g.row_block, tb, sh, sym0, st, pl);
      if (rc >= 0) return rc;
      return decode_stream_fused_cold(p, sizes[f], pre_off0, pre_len0, (uint32_t)g.row_block,
                                      reinterpret_cast<const uint32_t *>(tb.grp), tb.nd, sh, sym0, st,
                                      (uint32_t)g.max_sub, (uint32_t)g.lead_bits);
    }
    // Other widths: the same two paths, the lane's record read here (rows of a workgroup are
    // decoded one after the other: the loads of row i + 1 cannot be in flight under the prologue).
    const size_t ri = (size_t)f * g.rows + (size_t)r;
    const uint32_t *ps = ws.lane_start + ri * kDecThreads, *po = ws.lane_off + ri * (kDecThreads + kRecHdr);
    PreLane q;
    q.start = ps[tid]; q.off = po[tid]; q.nxt = po[tid + 1];
    q.nstart = tid + 1 < kDecThreads ? ps[tid + 1] : ~0u;
    q.tot = po[kDecThreads]; q.endrel = po[kDecThreads + 1]; q.valid = po[kDecThreads + 2]; q.rounds = po[kDecThreads + 3];
    const uint32_t off_r = ws.row_off[ri], len_r = ws.row_len[ri];
    // The row before ends by reading sh->err / sh->endbit with no barrier behind the reads: a slow
    // wavefront must not meet this row's reset while it still decides that one.
    if (i > 0) __syncthreads();
    if (tid == 0) { sh->err = 0; sh->endbit = ~0ull; }
    __syncthreads();
    uint32_t *st = ws.stats + ((size_t)f * (g.rows + 1) + r + 1) * 8;
    const int rc = decode_row_recorded(p, sizes[f], off_r, len_r, (uint32_t)g.row_block, tb, sh, sym0 + (size_t)i * rb16, st, q);
    if (rc >= 0) return rc;
    return decode_stream_fused_cold(p, sizes[f], off_r, len_r, (uint32_t)g.row_block,
                                    reinterpret_cast<const uint32_t *>(tb.grp), tb.nd, sh, sym0 + (size_t)i * rb16, st,
                                    (uint32_t)g.max_sub, (uint32_t)g.lead_bits);
  };
  int bad = 0;
  if constexpr (COLS == 512) {
    bad = decode_row(0);
  } else {
#pragma unroll 1
    for (int i = 0; i < nr && !bad; ++i) bad = decode_row(i);
  }
  if (bad) {   // uniform: every lane gets the same verdict
    if (tid == 0) atomicMax(&df->status, fmt_err(7, 1));
    return;
  }

  const long long c_p2 = clock64();
  // What the workgroup that takes this CU next will ask for first -- the packed bytes of the row 256
  // workgroups on (workgroups go to the XCDs round robin, so that one shares this one's L2) -- is
  // touched now, a line per lane of wavefronts 1..5: its first steps then wait for the L2 instead of
  // the HBM (decode of 128 frames 10.13 -> 9.95 ms; touching that row's lane record as well gains
  // nothing).  Loads nobody reads: the register is kept out of the compiler's hands until the
  // explicit wait in front of the pixel stores (transform_store_pair).
  uint32_t pf_a = 0;
  bool pf_on = false;
  {
    // (next_lin: the grid element this workgroup -- or its successor on this CU -- takes next)
    const int fn = (int)(next_lin / (uint32_t)gx), rn = r0 + (int)(next_lin % (uint32_t)gx) * rpw;
    pf_on = g.prefetch_rows != 0 && fn < gy && rn < r1;
    if (pf_on) {
      const int wv = tid >> 6, ln = tid & 63;
      // (how many bytes: this workgroup's own rows are the best guess -- 4096 pixels: the row's length
      // is at hand; other widths: the frame's mean)
      const uint32_t guess = COLS == 512 ? pre_len0 : (uint32_t)((unsigned long long)sizes[f] * (uint32_t)nr / (uint32_t)g.rows);
      const uint32_t o = 128u * (uint32_t)((wv - 1) * 64 + ln);
      if (wv >= 1 && wv <= 5 && o < guess + 256u) {
        // Never beyond that frame's stream: its rows may be shorter than this one's, and a frame
        // that failed to parse has no index at all (whatever the slot holds is compared, not trusted).
        const unsigned long long at = (unsigned long long)ws.row_off[(size_t)fn * g.rows + (size_t)rn] + o;
        if (at + 4ull <= (unsigned long long)sizes[fn]) {
          const uint8_t *a = packed + (size_t)fn * in_stride + at;
          const uint8_t *al = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(a) & ~(uintptr_t)3);
          asm volatile("global_load_dword %0, %1, off" : "=v"(pf_a) : "v"(al) : "memory");
        }
      }
    }
  }
  const int ycbcr = df->ycbcr;
  const int cols = COLS > 0 ? COLS : g.cols;
  // ---- phase 2: inverse transform, colour inverse and stores ----
  // Two adjacent lanes share a tile (transform_store_pair).  The decoded symbols
  // stay read-only in LDS: no barrier, no second pass over them.
  uint8_t *img;
  if constexpr (TENS) img = out_frames + (size_t)f * ((size_t)g.W * g.H * (size_t)(td->co * tens_elem_size(td->dtype)));
  else if constexpr (PITCH) img = dst_frame(out_frames, pd, f);
  else if constexpr (PLANES) img = out_frames + (size_t)f * ((size_t)g.W * g.H * (size_t)plane_count(pc->mask));
  else img = out_frames + (size_t)f * ((size_t)g.W * g.H * g.C);
  const int per_row = ((cols + 31) >> 5) * 64;   // whole wavefronts: a lane pair never straddles rows
  // (PYR: level 0 only where it is wanted -- uniform, a scalar load)
  bool want0 = true;
  if constexpr (PYR) want0 = pm->level[0] != nullptr;
  HIMG_SPAN_BEGIN("dec.transform");
#pragma unroll 1
  for (int it = tid; want0 && it < per_row * nr; it += kDecThreads) {
    const int i = COLS == 512 ? 0 : it / per_row, il = it - i * per_row;
    // A lane pair beyond the row's last tile (widths that are not a multiple of 256 pixels)
    // transforms the last tile once more and stores nothing: no exec-masked region around
    // the transform (with compile-time strides it cost 50 VGPR spills at 1920 pixels).
    const bool in_row = pair_tile(il) < cols;
    transform_store_pair<COLS, COLS != 0, false, TENS, PITCH, PLANES>(g, cols, sym0 + (size_t)i * rb16, low, s_unmap, s_shift, s_shiftp, ycbcr,
                                            in_row ? pair_tile(il) : cols - 1, pair_half(il), rb + i, img,
                                            COLS == 512 ? pre_lr : nullptr, in_row, pf_on && it == tid, pf_a,
                                            nullptr, 0, td, pd, pc);
  }
  HIMG_SPAN_END("dec.transform");
  if constexpr (PYR) {
    // Without level 0 no wavefront has met the wait for its touch load (transform_store_pair's).
    if (pf_on && !want0) asm volatile("s_waitcnt vmcnt(0)" ::"v"(pf_a) : "memory");
    // The 1/2- and 1/4-scale levels, behind the full-resolution loop: its registers are dead, the
    // symbols still read-only in LDS (the next row's barrier stands in front of their clear).  An
    // item is (part, row, tile) with the tile fastest: neighbouring lanes take neighbouring tiles,
    // so that a wavefront's stores of an output row are contiguous.  Part 0 is a tile's 4 x 4 at 1/2
    // scale -- in one pass: k_dec_scaled's two halves gather and transform the tile's sixteen symbols
    // twice to stay within 64 registers, which this kernel has no need of --, part 1 its 2 x 2 at 1/4
    // (4096-pixel rows: 512 + 512 items, one for every lane).
    uint8_t *const l1 = pm->level[1], *const l2 = pm->level[2];
    const int nt = cols * nr;
#pragma unroll 1
    for (int j = (l1 ? 0 : nt) + tid; j < (l2 ? 2 * nt : nt); j += kDecThreads) {
      const int part = j >= nt ? 1 : 0, t = j - part * nt;
      const int i = COLS == 512 ? 0 : t / cols, u = t - i * cols;
      const uint8_t *sy = sym0 + (size_t)i * rb16 + u;
      if (part == 0) pyr_tile_part<0>(g, cols, 64 * cols, sy, low, s_unmap, s_shift, ycbcr, u, rb + i, f, l1);
      else pyr_tile_part<1>(g, cols, 64 * cols, sy, low, s_unmap, s_shift, ycbcr, u, rb + i, f, l2);
    }
  }
  // A wavefront without a transform iteration (per_row * nr < 1024: narrow rows in a frame's last
  // workgroup) has not met the wait for its touch load: it waits here, the register its own up to
  // the wait, before the persistent loop hands it the next row.  (4096-pixel rows: every lane
  // has an iteration.)
  if constexpr (COLS != 512) {
    if (pf_on && tid >= per_row * nr) asm volatile("s_waitcnt vmcnt(0)" ::"v"(pf_a) : "memory");
  }
  // Cycle stamps: the slowest wave counts (the SIMDs issue oldest-first, so the
  // first wave finishes long before the last one).
  if ((tid & 63) == 0) {
    const long long c_out = clock64();
    for (int i = 0; i < nr; ++i) {
      uint32_t *st = ws.stats + ((size_t)f * (g.rows + 1) + rb + i + 1) * 8;
      atomicMax(&st[2], (uint32_t)((c_out - c_p2) >> 4));   // transform + stores
      atomicMax(&st[3], (uint32_t)((c_out - c_in) >> 4));   // the whole workgroup
    }
  }
}


// The kernel: a workgroup takes the rows bx = blockIdx.x, blockIdx.x + gridDim.x, ... of the
// launch's (rows / rpw) x batch grid, frame after frame.  With as many workgroups as the GPU
// holds at once (launch_decode: one per CU) a CU does not wait for a new workgroup -- its LDS, its
// wavefronts, their arguments -- between two rows (~3.6 k of a row's 61 k cycles), and the next
// row's records are requested while the last wavefronts of this row still transform.
// A kernel-argument struct into registers, word by word (a struct in the constant address space has
// no copy constructor the host pass accepts).
template <class W, class T>
__device__ __forceinline__ void karg_copy(T *dst, const __attribute__((address_space(4))) T *src) {
  static_assert(sizeof(T) % sizeof(W) == 0 && alignof(T) >= alignof(W), "whole words");
  const __attribute__((address_space(4))) W *sw = (const __attribute__((address_space(4))) W *)src;
  W *dw = reinterpret_cast<W *>(dst);
#pragma unroll
  for (size_t i = 0; i < sizeof(T) / sizeof(W); ++i) dw[i] = sw[i];
}
struct RowArgs {
  Geom g;
  DecWs ws;
  const uint8_t *packed;
  size_t in_stride;
  const uint32_t *sizes;
  uint8_t *out_frames;
  int r0, r1, rpw, gx, gy, next_dist;
};
// (The arguments are read from the kernel-argument segment anew for every row, through a pointer
// the compiler cannot see through: read once in front of the loop they all stay live across the
// body -- 104 scalar registers spilled instead of 36, the row kernel 9 % slower.)
// The kernel's five forms share the loop, dec_body_row_loop.inc; a form is its argument struct --
// RowArgs itself, or RowArgs followed by the form's descriptor --, its four flags and HIMG_ROW_A,
// the RowArgs inside the struct.  row_td / row_pd / row_pm / row_pc: the descriptor a form's struct carries.
struct RowArgsT {
  RowArgs a;
  TensDesc t;
};
struct RowArgsP {
  RowArgs a;
  DstDesc d;
};
struct RowArgsM {
  RowArgs a;
  PyrDesc m;
};
struct RowArgsC {
  RowArgs a;
  PlaneDesc c;
};
template <class K> __device__ __forceinline__ TensK row_td(K) { return nullptr; }
template <class K> __device__ __forceinline__ DstK row_pd(K) { return nullptr; }
template <class K> __device__ __forceinline__ PyrK row_pm(K) { return nullptr; }
template <class K> __device__ __forceinline__ PlaneK row_pc(K) { return nullptr; }
__device__ __forceinline__ TensK row_td(const __attribute__((address_space(4))) RowArgsT *ka) { return &ka->t; }
__device__ __forceinline__ DstK row_pd(const __attribute__((address_space(4))) RowArgsP *ka) { return &ka->d; }
__device__ __forceinline__ PyrK row_pm(const __attribute__((address_space(4))) RowArgsM *ka) { return &ka->m; }
__device__ __forceinline__ PlaneK row_pc(const __attribute__((address_space(4))) RowArgsC *ka) { return &ka->c; }

template <int COLS>
__global__ __launch_bounds__(kDecThreads) void k_dec_row_fused(RowArgs) {
  typedef RowArgs KA;
  constexpr bool kRowTens = false, kRowPitch = false, kRowPyr = false, kRowPlanes = false;
#define HIMG_ROW_A(ka) (*(ka))
#include "dec_body_row_loop.inc"
#undef HIMG_ROW_A
}

// k_dec_row_fused_t: the same kernel in its tensor form.  Its arguments are RowArgs -- unchanged, the
// uint8 kernels keep their code -- followed by the descriptor, which stays in the kernel-argument
// segment: the transform reads scale and bias there, per row and at the conversion, so that nothing
// of it is live across the row loop or the entropy phase.
#define HIMG_ROW_A(ka) ((ka)->a)
template <int COLS>
__global__ __launch_bounds__(kDecThreads) void k_dec_row_fused_t(RowArgsT) {
  typedef RowArgsT KA;
  constexpr bool kRowTens = true, kRowPitch = false, kRowPyr = false, kRowPlanes = false;
#include "dec_body_row_loop.inc"
}

// k_dec_row_fused_p: the same kernel in its pitched form.  RowArgs -- unchanged -- followed by the
// destination descriptor, which stays in the kernel-argument segment: the frame's origin is read
// where the transform phase begins, the pitch and the stride at the stores.
template <int COLS>
__global__ __launch_bounds__(kDecThreads) void k_dec_row_fused_p(RowArgsP) {
  typedef RowArgsP KA;
  constexpr bool kRowTens = false, kRowPitch = true, kRowPyr = false, kRowPlanes = false;
#include "dec_body_row_loop.inc"
}

// k_dec_row_fused_m: the same kernel in its pyramid form.  RowArgs -- unchanged, out_frames level 0 --
// followed by the levels' descriptor, which stays in the kernel-argument segment: the pointers are
// read behind the entropy phase, where the stores begin.
template <int COLS>
__global__ __launch_bounds__(kDecThreads) void k_dec_row_fused_m(RowArgsM) {
  typedef RowArgsM KA;
  constexpr bool kRowTens = false, kRowPitch = false, kRowPyr = true, kRowPlanes = false;
#include "dec_body_row_loop.inc"
}

// k_dec_row_fused_c: the same kernel in its planes form.  RowArgs -- unchanged -- followed by the
// plane mask, which stays in the kernel-argument segment: it is read where the transform phase begins
// (the frame's size), in front of the transform (which steps run) and at the stores.
template <int COLS>
__global__ __launch_bounds__(kDecThreads) void k_dec_row_fused_c(RowArgsC) {
  typedef RowArgsC KA;
  constexpr bool kRowTens = false, kRowPitch = false, kRowPyr = false, kRowPlanes = true;
#include "dec_body_row_loop.inc"
}
#undef HIMG_ROW_A

// ---------------------------------------------------------------------------
// k_row_count: the fixpoint rounds of every FRES block row, on their own.  They
// need no symbol storage (tables + the row's payload instead of the row's 128 KiB
// of symbols), so two workgroups share a CU at 8 waves per SIMD.  Output per lane:
// its first owned token and the exclusive prefix of the symbol counts; the fused
// kernel then goes straight to its write pass.
//   * a workgroup walks kRowsPerCount consecutive rows of one frame: the 28 KiB of
//     decode tables are loaded once for all of them (they were 17 % of a
//     one-row workgroup's cycles);
//   * the row's payload is staged in LDS (coalesced 4-byte loads) and the lanes'
//     bit windows refill from there;
//   * nothing is fenced at the end: the consumer is a later kernel.  (The
//     release fence + barrier that used to close the kernel wrote back L2 and cost
//     20 % of its duration.)
// ---------------------------------------------------------------------------
constexpr int kRowsPerCount = 4;

// Exclusive scan of a 32-bit value over the 1024-thread workgroup (DPP-free:
// 6 shuffles + one LDS exchange).
__device__ __forceinline__ uint32_t block_scan_u32d(uint32_t v, uint32_t *sm, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) sm[wave] = incl;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kDecThreads / 64; ++w) {
    const uint32_t x = sm[w];
    if (w < wave) pre += x;
    tot += x;
  }
  *total = tot;
  return pre + incl - v;
}

// QTR: three more boundaries inside every lane's range (lean_fixpoint's marks at 1/4, 1/2,
// 3/4) go to l_q ([6][kDecThreads]: positions, then output offsets), and the quarter
// records that hold the first symbol of every 128 KiB window of the row's symbols to the
// header (k_row_window then has 1024 sub-sequences per window to walk instead of 256).
template <class RD, bool QTR = false>
__device__ __forceinline__ void row_count_one(RD &rd, const GrpTables &tb, StreamShared *sh, uint32_t *sm32,
                                              uint32_t rel0, uint32_t rem, uint32_t sb, uint32_t lead_bits,
                                              uint32_t *l_start, uint32_t *l_off, uint32_t *rc, long long c_in,
                                              uint32_t *l_q = nullptr, uint32_t out_size = 0, uint32_t window = 0) {
  const int tid = threadIdx.x;
  const uint32_t rel_end = rel0 + rem;
  const SubGrid sg = sub_grid(rel0, rem, sb, tid);
  const uint32_t my_b0 = sg.b0, lim = sg.lim;
  const bool active = sg.active;
  const int last_active = sg.last_active;
  uint32_t start = active ? my_b0 : rel_end, endpos = start, cnt = 0, rounds = 0;
  long long c_phase[2] = {0, 0};
  const long long c_fix0 = clock64();
  uint32_t mark[3] = {0, 0, 0}, mcnt[3] = {0, 0, 0};
  if (QTR) {
    const uint32_t q = active ? (lim - my_b0) >> 2 : 0u;
    mark[0] = start + q; mark[1] = start + 2u * q; mark[2] = start + 3u * q;
    lean_fixpoint<true, RD, 0, 3>(rd, tb, sh, rel0, active, lim, &start, &endpos, &cnt, &rounds, false, lead_bits, nullptr,
                                  c_phase, nullptr, mark, mcnt);
  } else {
    lean_fixpoint<true>(rd, tb, sh, rel0, active, lim, &start, &endpos, &cnt, &rounds, false, lead_bits, nullptr, c_phase);
  }
  const long long c_fix1 = clock64();
  // 32-bit scan: a lane's count is clamped to 2^22 - 1, more than a whole row holds
  // (the caller only comes here for rows below 2^22 symbols), so 1024 of them cannot
  // wrap, valid streams are exact, and a lane that claims more still overruns the
  // block in the write pass and is rejected there like before.
  uint32_t tot;
  const uint32_t cc = min(cnt, 0x3fffffu);
  const uint32_t off = block_scan_u32d(cc, sm32, &tot);
  l_start[tid] = start - rel0;
  l_off[tid] = off;
  if (QTR) {
    uint32_t o[5];
    o[0] = off; o[4] = off + cc;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k + 1] = off + min(mcnt[k], cc);
      l_q[k * kDecThreads + tid] = mark[k] - rel0;
      l_q[(3 + k) * kDecThreads + tid] = o[k + 1];
    }
    // The quarter record that holds the first symbol of window w (w >= 1).
    if (window && cc) {
      for (uint32_t w = (o[0] + window - 1u) / window; w * window < o[4] && w * window < out_size && w < (uint32_t)(kRecHdr - kRecWin); ++w) {
        if (w == 0) continue;
        const uint32_t X = w * window;
        int k = 0;
#pragma unroll
        for (int j = 1; j < 4; ++j) if (X >= o[j]) k = j;
        l_off[kDecThreads + kRecWin + w] = 4u * (uint32_t)tid + (uint32_t)k;
      }
    }
  }
  if (tid == last_active) l_off[kDecThreads + 1] = endpos - rel0;
  if (tid == 0) {
    l_off[kDecThreads] = tot;
    l_off[kDecThreads + 3] = rounds | (min(sh->dbg[0], 4095u) << 8) | (min(sh->dbg[1], 4095u) << 20);
    l_off[kDecThreads + 4] = QTR ? 1u : 0u;
    l_off[kDecThreads + 2] = 1;   // (no fence: the consumer is a later kernel)
  }
  if ((tid & 63) == 0 && rc) {   // cycles / 16, slowest wave of the workgroup
    atomicMax(&rc[0], (uint32_t)((c_fix0 - c_in) >> 4));            // tables / payload staging
    atomicMax(&rc[1], (uint32_t)(c_phase[0] >> 4));                 // lead-in
    atomicMax(&rc[2], (uint32_t)(c_phase[1] >> 4));                 // ... to the end of round 1
    atomicMax(&rc[3], (uint32_t)((c_fix1 - c_fix0) >> 4));          // the whole fixpoint
    atomicMax(&rc[4], (uint32_t)((clock64() - c_in) >> 4));         // the row
  }
}

// LDSPAY: the row's payload is staged in LDS (rows of up to 36 KiB -- every shape
// the fused row kernel serves); otherwise (wide rows, generic path) the lanes read
// it in place.  The body (dec_body_row_count.inc) is also the region decode's per-frame
// form's, k_region_count.
template <bool LDSPAY>
__global__ __launch_bounds__(kDecThreads, 8) void k_row_count(Geom g, DecWs ws, const uint8_t *packed,
                                                           size_t in_stride, const uint32_t *sizes,
                                                           int r0, int r1, int rows_per_wg) {
#include "dec_body_row_count.inc"
}

// ---------------------------------------------------------------------------
// k_row_count_w: the same records (every one of the 1024 lanes of a row kernel: its first
// owned token and the exclusive prefix of the symbol counts), computed by ONE WAVEFRONT
// per row -- for batches, where there are rows enough to fill the GPU that way.  The
// wavefront takes the row kernel's lanes 64 at a time (phase j: lanes 64 j .. 64 j + 63,
// a contiguous 2 KiB of the payload, read in place): speculative lead-in, count, then
// the chain is made exact among the 64 (a lane starts where its left neighbour ended:
// one DPP move per round instead of an LDS exchange and two workgroup barriers; a lane
// whose guess was wrong walks to its re-join point again, 64 bits), and the
// prefix of the counts is a wave scan on top of the phases before.  Lane 0 of a phase
// starts where lane 63 of the phase before ended: exact, like the first lane of a chunk.
// No staging of the payload (staging a phase's 2.3 KiB in LDS per wavefront was measured:
// no faster -- the kernel is bound by the decode steps themselves), no 1024-lane scans,
// sixteen rows share one load of the decode tables.
// ---------------------------------------------------------------------------
constexpr int kCountRowsW = kDecThreads / 64;   // rows per workgroup (one per wavefront)

// Wavefront scan / shift on the DPP path (one VALU operation per step where __shfl_up is a
// ds_bpermute with its address arithmetic, a wait and a select).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_from_d(uint32_t identity, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_scan_add_dpp(uint32_t v) {   // inclusive; lane 63: the total
  v += dpp_from_d<0x111, 0xf>(0, v);   // row_shr:1
  v += dpp_from_d<0x112, 0xf>(0, v);   // row_shr:2
  v += dpp_from_d<0x114, 0xf>(0, v);   // row_shr:4
  v += dpp_from_d<0x118, 0xf>(0, v);   // row_shr:8
  v += dpp_from_d<0x142, 0xa>(0, v);   // row_bcast:15
  v += dpp_from_d<0x143, 0xc>(0, v);   // row_bcast:31
  return v;
}
// Lane l gets lane l - 1's v, lane 0 gets `first` (wave_shr:1).
__device__ __forceinline__ uint32_t wave_shr1_dpp(uint32_t first, uint32_t v) {
  return dpp_from_d<0x138, 0xf>(first, v);
}

// A piece of the payload staged in LDS, read ON DEMAND: a step fetches the 32 stream bits
// at its position with one ds_read2_b32 and one v_alignbit instead of keeping a 64-bit
// register window alive (the refill of ReaderT -- ten instructions with a 64-bit shift
// and a global load -- is executed by the whole wavefront whenever one of its 64 lanes
// runs low, i.e. on almost every step).  A step consumes at most kLutBits + 14 = 25 bits.
// Layout: the lanes of a wavefront read at a stride of one sub-sequence (8 dwords for
// 256 bits) and advance at about the same pace, which in a plain copy is an 8-way bank
// conflict on every read.  The piece is therefore stored in blocks of 33 dwords -- 32 of
// the payload, then a COPY of the next block's first dword -- so that dword w sits at
// w + w / 32 (the lane stride becomes co-prime with the 32 banks) and the pair
// (w, w + 1) is adjacent for every w.
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));   // two dwords at a dword-aligned address: ds_read2_b32
struct LdsBits {
  uint32_t base;   // LDS byte address of the dword that holds bit 0
  __device__ __forceinline__ uint32_t window(uint32_t pos) const {
    const uint32_t w = pos >> 5;
    const uint32_t a = base + ((w + (w >> 5)) << 2);
    const u32x2 x = *(const __attribute__((address_space(3))) u32x2_a4 *)(uintptr_t)a;
    return __builtin_amdgcn_alignbit(x.y, x.x, pos);   // (the hardware takes pos[4:0])
  }
};
// A lane's OWN piece of the payload (k_row_count_w's stretches): kLaneWords dwords from the dword
// of the lane's current position, at a stride that is co-prime with the 32 banks.  What a walk
// of one sub-sequence from there can touch: up to 31 bits of alignment, the sub-sequence (at
// most kStageSubBits), and a last step that starts on its last bit and takes a whole token
// with it (46 bits: a 32-bit code and 14 extra bits) -- bit 31 + 320 + 45 lies in dword 12.
// ds_read2 also fetches the dword behind the one it needs: for the last dword of a piece that
// is the next lane's first one (the buffer ends with a spare dword), whose bits nothing reads.
constexpr uint32_t kLaneWords = 13;
constexpr uint32_t kLaneAlloc = (64u * kLaneWords + 1u + 3u) & ~3u;
struct LaneBits {
  uint32_t base;   // LDS byte address the piece's first dword WOULD have if the piece began at bit 0
  __device__ __forceinline__ uint32_t window(uint32_t pos) const {
    const uint32_t a = base + ((pos >> 5) << 2);
    const u32x2 x = *(const __attribute__((address_space(3))) u32x2_a4 *)(uintptr_t)a;
    return __builtin_amdgcn_alignbit(x.y, x.x, pos);
  }
};
constexpr uint32_t kStageSubBits = 320;                                    // longest sub-sequence the staged form takes
constexpr uint32_t kStageWords = 64u * kStageSubBits / 32u + 32u;          // payload dwords of one phase: 64 sub-sequences + slack
constexpr uint32_t kStageAlloc = (kStageWords + kStageWords / 32u + 3u) & ~3u;  // the same in blocks of 33
static_assert(kStageWords % 32 == 0, "whole blocks");

// 64 stream bits in a register pair, for walk_token (no refill: one token at most).
struct BitWin64 {
  unsigned long long win;
  __device__ __forceinline__ void consume(int n) { win >>= n; }
  __device__ __forceinline__ void refill() {}
};

// The GROUPS that start in [pos, lim), from the staged payload (lean_count<.., GRP = true>
// over an LdsBits): where the last one ends, how many symbols they produce.
template <class BITS>
__device__ __forceinline__ void grp_count_lds(const BITS &bits, const GrpTables &t, uint32_t pos, uint32_t lim,
                                              uint32_t *endpos, uint32_t *count) {
  uint32_t c = 0;
  if (pos < lim) {
    bool bad = false;
    const uint32_t TM = (uint32_t)kLutBits;   // (index BITS: the address is a v_bfe and a v_lshl_add)
    const uint32_t TB = lds_addr(t.gy);
    const uint32_t XOFF = (uint32_t)kTabEntries * 4u;   // from a step word to its .x
    uint32_t tm = TM, tb = TB;   // which table the next step indexes (lean_count: long codes take two steps)
    auto step = [&]() {
      uint32_t win = bits.window(pos);
      uint32_t a;   // (index << 2) + tb in ONE instruction (the compiler splits it: shift, add)
      asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(a) : "v"(__builtin_amdgcn_ubfe(win, 0u, tm)), "v"(tb));
      uint32_t y = lds_ld32(a);
      uint32_t ntm = TM, ntb = TB;
      if (__builtin_expect(y == 0, 0)) {
        const uint32_t x = lds_ld32(a + XOFF);
        if ((x >> 31) && tm == TM) {
          ntm = x & 255u;
          ntb = TB + (((1u << kLutBits) + ((x >> 8) & 0xffffu)) << 2);
          y = (uint32_t)kLutBits | ((uint32_t)kLutBits << 27);
        } else {
          // Neither table resolves it: the tree walk, over a register window at pos.
          BitWin64 rd;   // 64 bits: the deepest code the walk follows is 32
          rd.win = (unsigned long long)win | ((unsigned long long)bits.window(pos + 32u) << 32);
          const int base = tm == TM ? 0 : kLutBits;
          uint32_t len, by;
          y = walk_token(rd, t, x, base, &len, &by, &bad);
          pos += len - (uint32_t)base;
          win = bits.window(pos);
        }
      }
      tm = ntm; tb = ntb;
      const uint32_t extra = __builtin_amdgcn_ubfe(win, y, y >> 5);
      pos += y >> 27;
      c += ((y >> 10) & 511u) + extra;
    };
    LoopCount lc;
    while (pos < lim) { HIMG_REGION_BEGIN("dec.count"); step(); lc.step(); HIMG_REGION_END("dec.count"); }
    lc.done(1);
    if (tm != TM) step();   // the loop ended between the two steps of a long code
  }
  *endpos = pos;
  *count = c;
}

// Rows whose sub-sequences are at most kStageSubBits bits long (4096-pixel rows up to
// ~2.4 bits per symbol): every phase's piece of the payload goes to LDS first -- coalesced
// 16-byte loads -- and the walks read it on demand (grp_count_lds); longer rows are read in
// place through register windows (wave-uniform choice per row).  The body (dec_body_row_count_w.inc)
// is also the region decode's per-frame form's, k_region_count_w.
// NQ > 1: a lane owns a STRETCH of NQ consecutive sub-sequences (the body explains); NQ = 1 is
// the form of a sub-sequence per lane, which the region and prefix decodes keep.  k_row_count_w is
// the form the decoder launches by default, k_row_count_wn the others (HIMG_OPT_COUNT_STRETCH).
constexpr int kCountStretch = 4;
__global__ __launch_bounds__(kDecThreads, 8) void k_row_count_w(Geom g, DecWs ws, const uint8_t *packed,
                                                               size_t in_stride, const uint32_t *sizes,
                                                               int r0, int r1) {
  constexpr int NQ = kCountStretch;
#include "dec_body_row_count_w.inc"
}
template <int NQ>
__global__ __launch_bounds__(kDecThreads, 8) void k_row_count_wn(Geom g, DecWs ws, const uint8_t *packed,
                                                                size_t in_stride, const uint32_t *sizes,
                                                                int r0, int r1) {
#include "dec_body_row_count_w.inc"
}
static_assert((31u + kStageSubBits + 45u) / 32u < kLaneWords, "a sub-sequence and its overrun fit a lane's piece");
static_assert(64 * 8 <= kLaneAlloc && 64 * kCountStretch <= kLaneAlloc, "a phase's 64 NQ records pass through a wavefront's staging buffer");

// ---------------------------------------------------------------------------
// k_row_count_q: the records of a WIDE row (one that goes through k_row_window: wider than the
// LDS, e.g. the 16384-pixel rows of BASELINE config 4) -- FOUR per row-kernel lane, i.e. 4096
// sub-sequences per row, at the cost per step of k_row_count_w: the payload staged in LDS in
// blocks of 33 dwords and read on demand (15 VALU per step), where k_row_count<false> keeps a
// register window over global memory (28+, and 100 us per 1-Mbit row whatever the number of
// rows in flight: config-4 decode was bound by it).
// One workgroup per row.  Wavefront w takes sub-sequences [256 w, 256 w + 256) as four phases
// of 64 exactly like k_row_count_w takes a whole row (speculative lead-in, the chain inside a
// phase by DPP, a phase's first lane exact from the phase before); what is speculative here is
// where a WAVEFRONT's first sub-sequence starts.  The sixteen wavefronts then compare: wave w
// is right if it started where wave w - 1 ended (wave 0 is exact, the rest by induction);
// the lowest wave that is not walks its sub-sequences again from the exact position -- about
// one row in ten has such a wave (a 128-bit lead-in misses in < 1 % of the boundaries).
// Records: sub-sequence v is quarter v & 3 of lane v >> 2 in k_row_count<.., QTR>'s layout
// (lane_start / lane_off for quarter 0, lane_q for the others), flag 3 (boundaries of the
// write pass's chain of groups), and the index of the record that holds the first symbol of
// every 128 KiB window.
// ---------------------------------------------------------------------------
constexpr int kQPhases = 4;   // phases of 64 sub-sequences per wavefront: 16 x 4 x 64 = 4 x kDecThreads
// Where record q = 4 * lane + quarter lives (k_row_count<.., QTR>'s layout, k_row_window's rec_pos / rec_off).
__device__ __forceinline__ uint32_t *qrec_pos(uint32_t *l_start, uint32_t *l_q, uint32_t q) {
  const uint32_t t = q >> 2, k = q & 3u;
  return k == 0 ? l_start + t : l_q + (k - 1u) * kDecThreads + t;
}
__device__ __forceinline__ uint32_t *qrec_off(uint32_t *l_off, uint32_t *l_q, uint32_t q) {
  const uint32_t t = q >> 2, k = q & 3u;
  return k == 0 ? l_off + t : l_q + (2u + k) * kDecThreads + t;
}
__global__ __launch_bounds__(kDecThreads, 8) void k_row_count_q(Geom g, DecWs ws, const uint8_t *packed,
                                                               size_t in_stride, const uint32_t *sizes, int r0) {
  __shared__ __attribute__((aligned(16))) uint32_t gyx[2 * kTabEntries];
  __shared__ uint32_t nd[kMaxNodes + 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[kCountRowsW * kStageAlloc];
  __shared__ int s_flag;
  __shared__ uint32_t s_ws[kCountRowsW], s_we[kCountRowsW], s_wc[kCountRowsW], s_wl[kCountRowsW], s_bad;
  uint32_t *gy = gyx, *gx = gyx + kTabEntries;
  const int f = blockIdx.y, r = r0 + (int)blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  DecFrame *df = ws.frames + f;
  if (tid == 0) {
    const int w = df->parse_status == 0 ? df->walk_status : 0;   // (k_row_count's rule)
    if (w && blockIdx.x == 0) atomicMax(&df->status, w);
    s_flag = df->status | w;
  }
  __syncthreads();
  const int failed = s_flag;
  const size_t ri = (size_t)f * g.rows + (size_t)r;
  uint32_t *l_start = ws.lane_start + ri * kDecThreads;
  uint32_t *l_off = ws.lane_off + ri * (kDecThreads + kRecHdr);
  uint32_t *l_q = ws.lane_q + ri * (6 * kDecThreads);
  if (tid == 0) l_off[kDecThreads + 2] = 0;                                   // not usable until proven otherwise
  if (tid >= kRecWin && tid < kRecHdr) l_off[kDecThreads + tid] = ~0u;        // no window index yet
  const uint32_t pay_off = ws.row_off[ri], pay_len = ws.row_len[ri];
  const unsigned long long rem64 = 8ull * pay_len;
  uint32_t sb1 = (uint32_t)((rem64 + kDecThreads - 1) / kDecThreads);   // the row kernels' sub-sequence: one chunk?
  sb1 = (sb1 + 31u) & ~31u;
  sb1 = sb1 < kMinSubBits ? kMinSubBits : sb1;
  constexpr uint32_t NSUB = 4u * (uint32_t)kDecThreads;
  uint32_t sb = (uint32_t)((rem64 + NSUB - 1u) / NSUB);
  sb = (sb + 31u) & ~31u;
  sb = sb < kMinSubBits ? kMinSubBits : sb;
  // Several chunks or nothing to do (k_row_count's rule), or sub-sequences beyond the staging
  // buffer (more than ~2.4 bits per symbol of a 16384-pixel row): the record stays unusable
  // and k_dec_huff decodes the row on its own.
  if (failed || sb1 > (uint32_t)g.max_sub || rem64 == 0 || g.row_block >= (1 << 22) || sb > kStageSubBits) return;
  {   // the write pass's step words next to the long-code descriptors (k_row_count_w)
    const uint32_t *nodes = ws.nodes + ((size_t)f * 2 + 1) * (kMaxNodes + 1);
    const int nn = df->s[1].num_nodes;
    for (int k = tid; k < nn; k += kDecThreads) nd[k] = nodes[k];
    const uint4 *gg = reinterpret_cast<const uint4 *>(ws.grp + ((size_t)f * 2 + 1) * (1u << kLutBits));
    for (int k = tid; k < (1 << kLutBits) / 2; k += kDecThreads) {
      const uint4 q = gg[k];
      reinterpret_cast<uint2 *>(gx)[k] = make_uint2(q.x, q.z);
      reinterpret_cast<uint2 *>(gy)[k] = make_uint2(q.y, q.w);
    }
    const uint4 *gs = reinterpret_cast<const uint4 *>(ws.sub + ((size_t)f * 2 + 1) * kSubEntries);
    for (int k = tid; k < kSubEntries / 2; k += kDecThreads) {
      const uint4 q = gs[k];
      reinterpret_cast<uint2 *>(gx + (1 << kLutBits))[k] = make_uint2(q.x, q.z);
      reinterpret_cast<uint2 *>(gy + (1 << kLutBits))[k] = make_uint2(q.y, q.w);
    }
  }
  __syncthreads();
  GrpTables tb;
  tb.grp = nullptr; tb.gx = gx; tb.gy = gy; tb.nd = nd;
  const uint32_t rem = (uint32_t)rem64;
  GReader rd;
  const uint32_t rel0 = rd.attach(packed + (size_t)f * in_stride, sizes[f], 8ull * pay_off);
  const uint32_t rel_end = rel0 + rem;
  const uint32_t lead = (uint32_t)g.lead_bits;
  uint32_t *stage = s_stage + wave * kStageAlloc;
  LdsBits bits;
  bits.base = lds_addr(stage);
  uint32_t w_start = rel_end, w_end = rel_end, w_last = rel_end, w_cnt = 0, rounds = 0;
  // All four phases of this wavefront.  first0 / exact0: where its first sub-sequence starts,
  // exactly -- or its nominal start, the real one to be found by a lead-in like any lane's.
  // The records go out as they are found, offsets relative to the wavefront's first symbol.
  auto run_wave = [&](uint32_t first0, bool exact0) {
    uint32_t first = first0, base = 0;
    bool have_start = false;
#pragma unroll 1
    for (int j = 0; j < kQPhases; ++j) {
      const uint32_t v = 256u * (uint32_t)wave + 64u * (uint32_t)j + (uint32_t)lane;
      const uint32_t nb0 = v ? rel0 + v * sb : rel0;              // nominal range of sub-sequence v
      uint32_t nlim = rel0 + (v + 1u) * sb;
      if (nlim > rel_end) nlim = rel_end;
      const bool active = nb0 < rel_end;
      const uint32_t pb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)nb0);
      if (pb0 >= rel_end) {   // a phase beyond the payload: its sub-sequences own nothing
        *qrec_pos(l_start, l_q, v) = rem;
        *qrec_off(l_off, l_q, v) = base;
        continue;
      }
      const bool spec0 = j == 0 && !exact0;   // the phase's first lane looks for its start as well
      uint32_t sfrom = pb0;
      if (spec0) sfrom = pb0 - rel0 > lead ? pb0 - lead : rel0;
      if (first < sfrom) sfrom = first;         // (an exact start in front of the nominal one: the group before ran long)
      const uint32_t w0 = sfrom >> 5;
      const uint32_t shift = 32u * w0;          // positions below: relative to the first staged dword
      wave_lds_sync();   // the walks of the phase before are done with the buffer
      for (uint32_t k = (uint32_t)lane; 4u * k < kStageWords; k += 64u) {
        const uint32_t w = w0 + 4u * k;
        uint4 x;
        if (w + 3u <= rd.jmax) {
          const PackedU4 u = *reinterpret_cast<const PackedU4 *>(rd.w + w);
          x.x = u.x; x.y = u.y; x.z = u.z; x.w = u.w;
        } else {
          x.x = rd.ld(w); x.y = rd.ld(w + 1u); x.z = rd.ld(w + 2u); x.w = rd.ld(w + 3u);
        }
        uint32_t *d = stage + 4u * k + (k >> 3);   // blocks of 33 (LdsBits)
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
        if ((k & 7u) == 0u && k) d[-1] = x.x;
      }
      wave_lds_sync();
      const uint32_t b0 = nb0 - shift, lim = nlim - shift, lo0 = rel0 - shift, fst = first - shift;
      uint32_t start = active ? b0 : rel_end - shift;
      if (lane == 0 && active && !spec0) start = fst;
      if ((lane > 0 || spec0) && active && lead) {   // (lo0 may lie below zero in this frame of reference: differences only)
        uint32_t from = start - lo0 > lead ? start - lead : lo0;
        if (from < sfrom - shift) from = sfrom - shift;   // (not in front of what is staged)
        uint32_t guess, none;
        grp_count_lds(bits, tb, from, start, &guess, &none);
        start = guess;
      }
      uint32_t endpos = start, cnt = 0;
      bool dirty = active;
      uint32_t T = (active ? b0 : rel_end - shift) + kJoinBits;
      if (T > lim || T < b0) T = lim;
      uint32_t posT = ~0u, cT = 0;
      for (;;) {
        if (dirty) {
          uint32_t p1, c1;
          grp_count_lds(bits, tb, start, T, &p1, &c1);
          if (p1 == posT) {
            cnt = c1 + (cnt - cT);
          } else {
            uint32_t c2;
            grp_count_lds(bits, tb, p1, lim, &endpos, &c2);
            cnt = c1 + c2;
          }
          posT = p1;
          cT = c1;
        }
        // The chain: a lane starts where its left neighbour ended; the first lane of a
        // speculative phase keeps the start its lead-in found.
        const uint32_t lane0 = spec0 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)start) : fst;
        const uint32_t ns = wave_shr1_dpp(lane0, endpos);
        dirty = active && ns != start;
        if (active) start = ns;
        ++rounds;
        if (!__any(dirty ? 1 : 0)) break;
      }
      const uint32_t c = min(cnt, 0x3fffffu);
      const uint32_t incl = wave_scan_add_dpp(c);
      *qrec_pos(l_start, l_q, v) = active ? start + shift - rel0 : rem;
      *qrec_off(l_off, l_q, v) = base + incl - c;
      if (!have_start) { w_start = (uint32_t)__builtin_amdgcn_readfirstlane((int)(start + shift)); have_start = true; }
      base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      first = (uint32_t)__builtin_amdgcn_readlane((int)(active ? endpos + shift : rel_end), 63);
      // where the chain of the row's LAST sub-sequence ends (the header's `endrel`)
      const int la = 63 - __clzll((long long)__ballot(active ? 1 : 0));
      w_last = (uint32_t)__builtin_amdgcn_readlane((int)(endpos + shift), la);
    }
    w_end = first;
    w_cnt = base;
    if (!have_start) w_start = rel_end;
  };
  const uint32_t nom0 = wave ? rel0 + 256u * (uint32_t)wave * sb : rel0;   // this wavefront's first nominal start
  const bool w_active = nom0 < rel_end;
  run_wave(nom0, wave == 0);
  // ---- the wavefronts agree on the chain ----
#pragma unroll 1
  for (int it = 0; it < kCountRowsW + 1; ++it) {
    if (lane == 0) { s_ws[wave] = w_start; s_we[wave] = w_end; s_wc[wave] = w_cnt; s_wl[wave] = w_last; }
    if (tid == 0) s_bad = 0xffffu;
    __syncthreads();
    // (a wavefront beyond the payload has nothing to be wrong about)
    const bool ok = wave == 0 || !w_active || s_ws[wave] == s_we[wave - 1];
    if (!ok && lane == 0) atomicMin(&s_bad, (uint32_t)wave);
    __syncthreads();
    const uint32_t bad = s_bad;
    if (bad == 0xffffu) break;
    if ((uint32_t)wave == bad) run_wave(s_we[wave - 1], true);   // everything in front of it is final: again, exactly
    __syncthreads();   // (s_ws / s_we / s_bad are rewritten at the top)
  }
  // ---- the offsets become the row's; the record that holds the first symbol of every window ----
  uint32_t wbase = 0, total = 0, endrel = 0;
  for (int w = 0; w < kCountRowsW; ++w) {
    const uint32_t c = s_wc[w];
    if (w < wave) wbase += c;
    total += c;
    if (w == 0 || rel0 + 256u * (uint32_t)w * sb < rel_end) endrel = s_wl[w] - rel0;
  }
  wave_lds_sync();   // (this wavefront's own stores above, before it reads them back)
  __threadfence_block();
  const uint32_t out_size = (uint32_t)g.row_block;
#pragma unroll 1
  for (int j = 0; j < kQPhases; ++j) {
    const uint32_t v = 256u * (uint32_t)wave + 64u * (uint32_t)j + (uint32_t)lane;
    uint32_t *po = qrec_off(l_off, l_q, v);
    // (read back what this wavefront stored above: device-scope loads, past the vector L1)
    const uint32_t rel = __hip_atomic_load(po, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the next record of this wavefront closes the range (its last one: the wavefront's total)
    const uint32_t nrel = (j == kQPhases - 1 && lane == 63)
                              ? w_cnt : __hip_atomic_load(qrec_off(l_off, l_q, v + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t off = wbase + rel, c = nrel - rel;
    *po = off;
    if (c) {
      for (uint32_t w = (off + kRowWindow - 1u) / kRowWindow; w * kRowWindow < off + c && w * kRowWindow < out_size &&
                                                                 w < (uint32_t)(kRecHdr - kRecWin); ++w)
        if (w) l_off[kDecThreads + kRecWin + w] = v;
    }
    wave_lds_sync();   // (lane l + 1 has read record v + 1's relative offset before lane l + 1 rewrites it -- see below)
  }
  if (tid == 0) {
    l_off[kDecThreads] = total;
    l_off[kDecThreads + 1] = endrel;
    l_off[kDecThreads + 3] = rounds;
    l_off[kDecThreads + 4] = 1;   // four records per lane
    l_off[kDecThreads + 2] = 3;   // boundaries of the write pass's chain of groups (no fence: the consumer is a later kernel)
  }
}

// ---------------------------------------------------------------------------
// k_row_window: write pass of rows whose symbols do not fit the LDS (wider than 4224
// pixels), one workgroup per 128 KiB WINDOW of a row's symbols (a channel plane of a
// 16384-pixel row).  Every lane looks at its own record from k_row_count and decodes its
// sub-sequence if its symbols touch the window -- about a quarter of the lanes of a
// 16384-pixel row, the two at the edges for both neighbours --, OR-ing the literals
// into the zeroed window in LDS exactly like the fused row kernel; the window then
// leaves as 16-byte stores.  (Storing every group straight to a pre-zeroed plane in HBM
// -- 64 different cache lines per wave instruction -- was 3.5 ms for a 16384 x 16384 frame
// against 1.0 ms for the same walk without the stores, plus 0.4 ms to clear the plane.)
// Rows without a usable fixpoint from k_row_count are k_dec_huff's, as before.
// ---------------------------------------------------------------------------
struct WinShared { int flag, err; unsigned long long endbit; };
__global__ __launch_bounds__(kDecThreads) void k_row_window(Geom g, DecWs ws, const uint8_t *packed,
                                                            size_t in_stride, const uint32_t *sizes, int r0) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  LdsTables &T = *reinterpret_cast<LdsTables *>(smem);
  WinShared &sh = *reinterpret_cast<WinShared *>(smem + sizeof(LdsTables));
  uint8_t *win = smem + sizeof(LdsTables) + 64;          // kWinGuard + window + kWinGuard
  const int wi = blockIdx.x, r = r0 + (int)blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
  DecFrame *df = ws.frames + f;
  const size_t ri = (size_t)f * g.rows + r;
  const uint32_t *pre_start = ws.lane_start + ri * kDecThreads, *pre_off = ws.lane_off + ri * (kDecThreads + kRecHdr);
  const uint32_t *lq = ws.lane_q ? ws.lane_q + ri * (6 * kDecThreads) : nullptr;
  // Everything from global memory in front of the first barrier.
  const uint32_t tot = pre_off[kDecThreads], usable = pre_off[kDecThreads + 2];
  const bool quarters = lq != nullptr && pre_off[kDecThreads + 4] != 0;   // four records per lane (k_row_count for wide rows)
  const uint32_t pay_off = ws.row_off[ri], pay_len = ws.row_len[ri], ssize = sizes[f];
  const unsigned long long P1 = 8ull * pay_len;
  // Record q of the row (quarters: 4 * lane + k, else the lane): where its tokens start (bits
  // from the row's first) and its first symbol; the record behind it closes its range.
  const uint32_t nrec = quarters ? 4u * (uint32_t)kDecThreads : (uint32_t)kDecThreads;
  auto rec_pos = [&](uint32_t q) -> uint32_t {
    if (q >= nrec) return (uint32_t)P1;
    if (!quarters) return pre_start[q];
    const uint32_t t = q >> 2, k = q & 3u;
    return k == 0 ? pre_start[t] : lq[(k - 1u) * kDecThreads + t];
  };
  auto rec_off = [&](uint32_t q) -> uint32_t {
    if (q >= nrec) return tot;
    if (!quarters) return pre_off[q];
    const uint32_t t = q >> 2, k = q & 3u;
    return k == 0 ? pre_off[t] : lq[(2u + k) * kDecThreads + t];
  };
  const uint32_t out_size = (uint32_t)g.row_block;
  const uint32_t w0 = (uint32_t)wi * kRowWindow, w1 = min(w0 + kRowWindow, out_size);
  // The window's first record, from the row's index.  (Checked below by the lane that gets
  // it: a record that does not hold the window's first symbol -- stale words -- sends the
  // workgroup through all records instead.)
  uint32_t q0 = 0;
  if (quarters && wi > 0 && wi < kRecHdr - kRecWin) {
    const uint32_t c = pre_off[kDecThreads + kRecWin + wi];
    if (c < nrec) q0 = c;
  }
  uint32_t q = q0 + (uint32_t)tid;
  uint32_t st_rel = rec_pos(q), nst_rel = rec_pos(q + 1u), off = rec_off(q), nxt = rec_off(q + 1u);
  if (tid == 0) { sh.flag = (df->status || usable == 0) ? 1 : 0; sh.err = 0; sh.endbit = ~0ull; }
  load_dec_tables(ws, df, f, 1, &T);
  const uint32_t span = (w1 - w0) + kWinGuard;           // guard + window bytes
  {
    uint4 z;
    z.x = z.y = z.z = z.w = 0;
    for (uint32_t k = tid; k < (span + kWinGuard + 15u) / 16u; k += kDecThreads) reinterpret_cast<uint4 *>(win)[k] = z;
  }
  const int stale = __syncthreads_or((tid == 0 && q0 != 0 && !(off <= w0 && w0 < nxt)) ? 1 : 0);
  if (sh.flag) return;   // frame failed, or the row is k_dec_huff's
  if (stale) {           // (uniform) the index did not name the window's first record: from the row's first
    q = (uint32_t)tid;
    st_rel = rec_pos(q); nst_rel = rec_pos(q + 1u); off = rec_off(q); nxt = rec_off(q + 1u);
  }
  const GrpTables tb = tables_of(&T);
  GReader rd;
  const uint32_t rel0 = rd.attach(packed + (size_t)f * in_stride, ssize, 8ull * pay_off);
  const uint32_t rel_out = out_size - w0 + kWinGuard;    // the block's end, same origin
  // Rounds of 1024 consecutive records (one round with one record per lane; with quarters
  // one per window unless the window's symbols take more than a quarter of the payload).
  for (;;) {
    if (q < nrec) {
      const uint32_t lim = nst_rel < (uint32_t)P1 ? rel0 + nst_rel : rel0 + (uint32_t)P1;
      const uint32_t cnt = nxt - off;
      // The record's symbols [off, off + cnt) against the window; positions are handed to the
      // write loops relative to the window's guard (they wrap below zero in front of it:
      // the clip test is one unsigned compare).
      const bool inside = off + cnt < out_size, exact = !inside && off < out_size;
      const bool touches = cnt > 0 && off < w1 && off + cnt > w0;
      if (touches || (exact && wi == (int)((out_size - 1u) / kRowWindow))) {
        uint32_t end_bp = ~0u;
        const uint32_t op = off - w0 + kWinGuard;
        if (inside) {
          if (!lean_write<true>(rd, tb, rel0 + st_rel, lim, op, win, span, usable == 3u)) sh.err = 1;
        } else if (exact) {
          if (!exact_write<true>(rd, tb, rel0 + st_rel, lim, op, rel_out, win, &end_bp, span)) sh.err = 1;
          if (end_bp != ~0u) sh.endbit = (unsigned long long)(end_bp - rel0);
        }
      }
    }
    // Another round while the records behind this one can still reach the window.
    const uint32_t qn = q - (uint32_t)tid + (uint32_t)kDecThreads;   // (uniform)
    const int more = __syncthreads_or((tid == kDecThreads - 1 && q < nrec && nxt < w1) ? 1 : 0);
    if (!more || qn >= nrec) break;
    q = qn + (uint32_t)tid;
    st_rel = rec_pos(q); nst_rel = rec_pos(q + 1u); off = rec_off(q); nxt = rec_off(q + 1u);
  }
  __syncthreads();
  // The window leaves as 16-byte stores (row blocks and windows are multiples of 16).
  uint8_t *dst = ws.fres_sym + (size_t)f * ws.fres_stride + (size_t)r * g.row_block + w0;
  for (uint32_t k = tid; k < (w1 - w0) / 16u; k += kDecThreads)
    reinterpret_cast<uint4 *>(dst)[k] = reinterpret_cast<const uint4 *>(win + kWinGuard)[k];
  // accept / reject like UncompressStream (huffman_dec.cpp:361-417): by the workgroup of
  // the row's last window, whose lanes include the one that completes the block.
  if (tid == 0 && w1 == out_size) {
    int bad = sh.err;
    if (tot < out_size) bad = 1;   // ran out of payload before the block was full
    const unsigned long long E = sh.endbit;
    if (!bad && !(E <= P1 && E + 8 > P1 && E > 0)) bad = 1;
    if (bad) atomicMax(&df->status, fmt_err(7, 1));
  } else if (tid == 0 && sh.err) {
    atomicMax(&df->status, fmt_err(7, 1));
  }
}

// k_dec_zero: the LRES symbol planes (16-byte units) and the two diagnostics arrays,
// one launch instead of three memsets in front of every decode.
__global__ __launch_bounds__(256) void k_dec_zero(uint4 *sym, uint32_t n16, uint32_t *a, uint32_t na, uint32_t *b,
                                                  uint32_t nb) {
  uint4 z;
  z.x = z.y = z.z = z.w = 0;
  const uint32_t k0 = blockIdx.x * (256u * 4u) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t k = k0 + (uint32_t)j * 256u;
    if (k < n16) sym[k] = z;
  }
  const uint32_t stride_t = gridDim.x * 256u, t0 = blockIdx.x * 256u + threadIdx.x;
  for (uint32_t k = t0; k < na; k += stride_t) a[k] = 0;
  for (uint32_t k = t0; k < nb; k += stride_t) b[k] = 0;
}

// k_dec_status: copy the per-frame verdict out of the workspace.
__global__ void k_dec_status(DecWs ws, int32_t *status, int batch) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < batch) {
    const DecFrame *df = ws.frames + f;
    const int w = df->parse_status == 0 ? df->walk_status : 0;   // (merged by k_row_count already unless no row was asked for)
    status[f] = df->status > w ? df->status : w;
  }
}

// ---------------------------------------------------------------------------
// k_lres_preview: the 1/8-scale preview.  The low-res plane [C][rows][cols] of a frame is
// its preview with the channels apart: pixel p = v * cols + u of the preview is byte p of
// every channel plane, so the kernel interleaves C planes of rows * cols bytes -- four
// pixels per lane, ragged widths need nothing -- and applies the colour inverse
// (ycbcr.cpp:54-82: int16 arithmetic, clamp; channels 3.. as they are) where the frame's
// FRMT asks for it.  RGBA: one 16-byte store per lane (four dwords where the frame's
// output does not start on 16 bytes).  Frames with a verdict are skipped.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void ycc_to_rgb(uint32_t &c0, uint32_t &c1, uint32_t &c2) {
  const int y = (int)c0, cb = ((int)c1 << 1) - 255, cr = ((int)c2 << 1) - 255;
  const int gg = y - ((cb + cr + 2) >> 2), b = gg + cb, r = gg + cr;   // (no int16 overflow: |b|, |r| < 640)
  c0 = (uint32_t)clamp255d(r); c1 = (uint32_t)clamp255d(gg); c2 = (uint32_t)clamp255d(b);
}

__global__ __launch_bounds__(256) void k_lres_preview(Geom g, DecWs ws, uint8_t *out) {
  const int f = blockIdx.y;
  const DecFrame *df = ws.frames + f;
  if (df->status) return;
  const uint32_t npix = (uint32_t)g.rows * (uint32_t)g.cols;
  const uint32_t p0 = 4u * (blockIdx.x * 256u + threadIdx.x);
  if (p0 >= npix) return;
  const int C = g.C, ycc = df->ycbcr;
  const uint8_t *plane = ws.low + (size_t)f * ws.plane_stride;
  uint8_t *dst = out + (size_t)f * npix * (uint32_t)C;
  const uint32_t np = npix - p0 < 4u ? npix - p0 : 4u;
  uint32_t v[4][4];   // [pixel][channel]
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      v[k][c] = (c < C && (uint32_t)k < np) ? plane[(size_t)c * npix + p0 + k] : 0u;
  if (ycc) {
#pragma unroll
    for (int k = 0; k < 4; ++k) ycc_to_rgb(v[k][0], v[k][1], v[k][2]);
  }
  if (C == 4 && np == 4) {
    uint4 q;
    q.x = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[0][3] << 24);
    q.y = v[1][0] | (v[1][1] << 8) | (v[1][2] << 16) | (v[1][3] << 24);
    q.z = v[2][0] | (v[2][1] << 8) | (v[2][2] << 16) | (v[2][3] << 24);
    q.w = v[3][0] | (v[3][1] << 8) | (v[3][2] << 16) | (v[3][3] << 24);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst + 4u * p0);   // (4 * npix per frame: dword aligned)
    if (((uintptr_t)d & 15u) == 0) {
      *reinterpret_cast<uint4 *>(d) = q;
    } else {
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if ((uint32_t)k < np && c < C) dst[(size_t)(p0 + k) * C + c] = (uint8_t)v[k][c];
}

// ---------------------------------------------------------------------------
// k_dec_region: the window w x h at frame f's own origin (x_f, y_f) (RegionArgs::org) of every
// frame of the batch at full resolution, h x w x C interleaved bytes per frame.  Frame f touches
// block rows r0_f = y_f / 8 .. r1_f = ceil((y_f + h) / 8) and tile columns u0_f = x_f / 8 ..
// u1_f = ceil((x_f + w) / 8); for a fixed w x h these counts differ between frames by at most one.
// A workgroup per (column strip of sw tiles, touched block row, frame) -- the grid is sized by
// the batch's largest counts, and a workgroup past its frame's last row or last tile returns
// first thing: the row's count record (k_region_count / k_region_count_w over the frame's
// touched rows only, every row in one chunk: launch_region),
// then a write pass that keeps only the strip's symbols, [C][64][strip tiles] in LDS, then
// the transform of the strip's tiles and cropped stores.  Nothing of the row's symbols goes
// to HBM and no tile outside the rectangle is transformed.
//   * symbol layout: segment (c, k) of the row's [C][64][cols] symbols is `S` bytes of LDS, a
//     guard dword, the strip's tiles, at least four guard bytes: a group's 4 bytes OR-ed in at
//     a column within three of the strip lands its outside bytes on the guards (RegionWin::put);
//   * a lane whose recorded symbols hold no strip column does not walk; one that does stops
//     behind its last strip symbol -- unless the frame's tree has a leaf the reference rejects
//     (the only symbol a walk can fail on: the parse rejects trees deeper than the walk), so
//     that every symbol the reference reads is still checked.  The lane that completes the
//     block always walks its whole range: it carries the row's verdict;
//   * a row without a usable record (the count kernels leave only rows of 2^22 symbols or more
//     without one here): lane 0 walks the whole row with the reference's checks;
//   * the payload is read in place, bounded by the row's last dword.
// ---------------------------------------------------------------------------
struct RegionArgs {
  const int32_t *org;  // frame f's origin (x_f, y_f) at org[2 f], org[2 f + 1] (blockIdx.y = row - r0_f)
  int sw;              // tiles per column strip (blockIdx.x = strip, from u0_f on)
  int w, h;            // the window
  uint8_t *out;        // frame f's pixels at out + f * h * w * C
};
// One frame's rectangle (transform_store_region's crop).
struct RegionRect {
  int x, y, w, h;
};

// LDS of k_dec_region: decode tables, the row's verdict state, the row tables (DecFrame::row_tabs),
// then the symbol segments.
struct RegionShared {
  unsigned long long endbit;   // where the block became complete (relative to the payload)
  int flag, err;
};
struct RegionLayout {
  uint32_t tab, sh, rowtab, sym, seg, total;
};
__host__ __device__ inline RegionLayout region_layout(int C, int sw) {
  RegionLayout L;
  uint32_t o = 0;
  auto carve = [&](uint32_t bytes) { uint32_t r = o; o += (bytes + 15u) & ~15u; return r; };
  L.tab = carve((uint32_t)sizeof(LdsTables));
  L.sh = carve((uint32_t)sizeof(RegionShared));
  L.rowtab = carve(4u * kRowTabWords);
  L.seg = (((uint32_t)sw + 3u) & ~3u) + 8u;
  L.sym = carve(L.seg * 64u * (uint32_t)C);
  L.total = o;
  return L;
}

// The strip of a block row's symbols in LDS.  put(op, by): a group's bytes `by` at symbol op of
// the row.  Symbol op is column op % cols of segment op / cols; the group's bytes may reach into
// the next segment (up to three more for rows of fewer than four tiles).
struct RegionWin {
  uint32_t base;        // LDS address of segment 0
  uint32_t cols, u0, ww, seg, nseg;
  __device__ __forceinline__ void put(uint32_t op, uint32_t by) const {
    if (by == 0) return;   // (zeros are the clear's)
    const uint32_t s0 = op / cols;
    const int c0 = (int)(op - s0 * cols);
#pragma unroll 1
    for (uint32_t j = 0; j < 4u; ++j) {
      const int c = c0 - (int)(j * cols) - (int)u0;   // the group's first byte, relative to the strip
      if (c0 - (int)(j * cols) < -3 || s0 + j >= nseg) break;
      if (c >= -3 && c < (int)ww) {
        const uint32_t a = base + (s0 + j) * seg + (uint32_t)(4 + c);
        const unsigned long long v = (unsigned long long)by << (8u * (a & 3u));
        lds_or32(a & ~3u, (uint32_t)v);
        lds_or32((a & ~3u) + 4u, (uint32_t)(v >> 32));
      }
    }
  }
};

// One lane's walk over the tokens that start in [bp, lim), symbols from op on.  !EXACT: every
// symbol of the range lies inside the block; the walk ends at lim or once op passes `stop`.
// EXACT (exact_write_body): the lane in whose range the block completes -- whole groups while the
// block stays incomplete behind them, then token by token with the reference's end-of-block
// checks (huffman_dec.cpp:353-354,361-417); *end_bp = where the block became complete.
template <bool EXACT, class WIN = RegionWin>
__device__ __forceinline__ bool region_walk(GReader &rd, const GrpTables &t, uint32_t bp, uint32_t lim, uint32_t op,
                                            uint32_t stop, uint32_t out_size, const WIN &win, uint32_t *end_bp) {
  if (!(bp < lim) || op >= out_size) return true;
  rd.init(bp);
  bool bad = false;
  const int limk = (int)lim - kLutBits;
  while ((int)bp <= limk && op <= stop) {
    const GReader saved = rd;
    uint32_t nbits, cnt, by;
    bool gbad = false;
    lean_step<true>(rd, t, false, &nbits, &cnt, &by, &gbad);
    if (EXACT && (gbad || op + cnt >= out_size)) { rd = saved; break; }
    bad |= gbad;
    win.put(op, by);
    op += cnt;
    bp += nbits;
  }
  if (!EXACT) {
    while (bp < lim && op <= stop) {
      uint32_t nbits, cnt, by;
      lean_step<true>(rd, t, true, &nbits, &cnt, &by, &bad);
      win.put(op, by);
      op += cnt;
      bp += nbits;
    }
    rd.retire();
    return !bad;
  }
  bool ok = true;
  for (;;) {
    uint32_t nbits, cnt, by;
    lean_step<true>(rd, t, true, &nbits, &cnt, &by, &bad);
    if (bad || op + cnt > out_size) { ok = false; break; }   // a zero run overruns the block
    win.put(op, by);
    op += cnt;
    bp += nbits;
    if (op >= out_size) { *end_bp = bp; break; }
    if (!(bp < lim)) break;
  }
  rd.retire();
  return ok;
}

// The transform of one tile half (transform_store_pair's lane pair, generic channel count) for the
// region: the symbols at sym with segment stride `sstride`, the low-res corners from the frame's
// planes at the global tile u, and the stores cropped to the rectangle (row pitch w * C).
// TENS: the planar float output (TensDesc) -- img is frame f's [co][h][w] elements, row pitch w
// elements per plane, element stores (a window's rows are only element-aligned).
// PITCH: the pitched output (DstDesc) -- img is the window's origin pixel in frame f's destination
// picture (dst_frame), rows row_pitch apart, pixels pixel_stride apart: a dword per pixel where four
// channels meet 4-byte pixels, the C channel bytes otherwise.
template <bool TENS = false, bool PITCH = false>
__device__ __forceinline__ void transform_store_region(const Geom &g, int sstride, const uint8_t *sym,
                                                       const uint8_t *low, const int16_t *s_unmap,
                                                       const uint8_t *s_shift, const uint32_t *s_shiftp, int ycbcr,
                                                       int u, int s, int v, const RegionRect &ra, uint8_t *img,
                                                       bool store_ok, TensK td = nullptr, DstK pd = nullptr) {
  const int cols = g.cols, C = g.C;
  const int v2 = min(v + 1, g.rows - 1), u2 = min(u + 1, cols - 1);
  uint32_t QA[16], QB[16];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const int c = 2 * s + cc;
    uint32_t O[16];
    if (c < C) {
      const uint8_t *m = low + (size_t)c * g.rows * cols;
      const int chroma = (ycbcr && (c == 1 || c == 2)) ? 1 : 0;  // decoder.cpp:376
      const uint32_t lr0 = (uint32_t)m[(size_t)v * cols + u] | ((uint32_t)m[(size_t)v * cols + u2] << 8);
      const uint32_t lr8 = (uint32_t)m[(size_t)v2 * cols + u] | ((uint32_t)m[(size_t)v2 * cols + u2] << 8);
      tile_plane<0>(sym + (size_t)c * 64 * sstride, sstride, s_unmap, s_shift + chroma * 64, s_shiftp + chroma * 32,
                    lr0, lr8, O, nullptr);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) O[i] = 0;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (cc == 0) QA[i] = O[i];
      else QB[i] = O[i];
    }
  }
  uint32_t ch0[8], ch1[8], ch2[8], ch3[8];   // [r*2+h]: pixel row 4s+r, x = 4h..4h+3 (see transform_store_pair)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const auto ra_ = __builtin_amdgcn_permlane32_swap(QA[i], QA[8 + i], false, false);
    const auto rb_ = __builtin_amdgcn_permlane32_swap(QB[i], QB[8 + i], false, false);
    ch0[i] = ra_[0]; ch2[i] = ra_[1];
    ch1[i] = rb_[0]; ch3[i] = rb_[1];
  }
  if (!store_ok) return;
  // (PITCH: the pitch and the stride, read once here -- behind the transform, for the four rows)
  size_t row_pitch = (size_t)ra.w * C;
  int pstr = C;       // bytes from a pixel to the next
  if constexpr (PITCH) {
    const DstK pk = dst_at_use(pd);
    row_pitch = pk->row_pitch; pstr = pk->pixel_stride;
  }
  const bool word = C == 4 && pstr == 4;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int py = 8 * v + 4 * s + rr - ra.y;   // pixel row in the rectangle
    if (py < 0 || py >= ra.h) continue;
    if constexpr (TENS) {
      // A tile inside the window: eight consecutive elements per channel, one or two 16-byte stores at
      // whatever alignment the window gives them; a tile the window's left or right edge cuts: its
      // elements [lo, hi), one by one (tens_store8).
      uint32_t pc[4][2];   // [channel][h]: the bytes of x = 4h..4h+3
#pragma unroll
      for (int h = 0; h < 2; ++h)
        tens_planes(ch0[rr * 2 + h], ch1[rr * 2 + h], ch2[rr * 2 + h], ch3[rr * 2 + h], ycbcr, pc[0][h], pc[1][h],
                    pc[2][h], pc[3][h]);
      const int dtype = td->dtype, co = td->co;
      const size_t es = (size_t)tens_elem_size(dtype);
      // (ternaries, not min / max: more callers of those shared inline functions and the compiler emits
      // other code for the existing kernels that call them)
      const int px0 = 8 * u - ra.x, lo = px0 < 0 ? -px0 : 0, hi = ra.w - px0 < 8 ? ra.w - px0 : 8;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < co) {
          const float sc = td->scale[c], bi = td->bias[c];
          const long long e = ((long long)c * ra.h + py) * ra.w + px0;   // (px0 < 0 at the left edge: lo > 0)
          tens_store8<false>(img + e * (long long)es, pc[c][0], pc[c][1], sc, bi, dtype, lo, hi);
        }
      }
      continue;
    }
    uint8_t *drow = img + (size_t)py * row_pitch;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t q0 = ch0[rr * 2 + h], q1 = ch1[rr * 2 + h], q2 = ch2[rr * 2 + h], q3 = ch3[rr * 2 + h];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int px = 8 * u + 4 * h + k - ra.x;
        uint32_t c0 = (q0 >> (8 * k)) & 255u, c1 = (q1 >> (8 * k)) & 255u, c2 = (q2 >> (8 * k)) & 255u;
        const uint32_t c3 = (q3 >> (8 * k)) & 255u;
        if (px < 0 || px >= ra.w) continue;
        if (ycbcr) ycc_to_rgb(c0, c1, c2);   // ycbcr.cpp:54-82
        uint8_t *d = drow + (size_t)px * pstr;
        if (word) {
          *reinterpret_cast<uint32_t *>(d) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);   // (4 w C per row: dword aligned)
        } else {
          d[0] = (uint8_t)c0;
          if (C > 1) d[1] = (uint8_t)c1;
          if (C > 2) d[2] = (uint8_t)c2;
        }
      }
    }
  }
}

__global__ __launch_bounds__(kDecThreads) void k_dec_region(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                           const uint32_t *sizes, RegionArgs ra) {
  constexpr bool kRegionTens = false, kRegionPitch = false;
  constexpr bool kRegionConceal = false, kRegionMap = false;
  uint8_t *const cmap = nullptr;
  const int32_t *const smap = nullptr;
  int32_t *const wstat = nullptr;
  const TensK td = nullptr;
  const DstK pd = nullptr;
#include "dec_body_region.inc"
}

// k_dec_region_t: the same kernel in its tensor form -- frame f's [co][h][w] elements at
// ra.out + f * co * h * w elements, the crop of the full decode's tensor.  The arguments in one
// struct: the descriptor is read from the kernel-argument segment where the stores use it.
struct RegionArgsT {
  Geom g;
  DecWs ws;
  const uint8_t *packed;
  size_t in_stride;
  const uint32_t *sizes;
  RegionArgs ra;
  TensDesc t;
};
__global__ __launch_bounds__(kDecThreads) void k_dec_region_t(RegionArgsT a) {
  constexpr bool kRegionTens = true, kRegionPitch = false;
  constexpr bool kRegionConceal = false, kRegionMap = false;
  uint8_t *const cmap = nullptr;
  const int32_t *const smap = nullptr;
  int32_t *const wstat = nullptr;
  const DstK pd = nullptr;
  const Geom &g = a.g;
  const DecWs &ws = a.ws;
  const uint8_t *packed = a.packed;
  const size_t in_stride = a.in_stride;
  const uint32_t *sizes = a.sizes;
  const RegionArgs &ra = a.ra;
  const TensK td = &((const __attribute__((address_space(4))) RegionArgsT *)__builtin_amdgcn_kernarg_segment_ptr())->t;
#include "dec_body_region.inc"
}

// k_dec_region_p: the same kernel in its pitched form -- frame f's window w x h at the origin
// d.org[2 f], d.org[2 f + 1] of its destination picture (ra.out: the first picture; ra.org stays the
// window's origin in the decoded picture).
struct RegionArgsP {
  Geom g;
  DecWs ws;
  const uint8_t *packed;
  size_t in_stride;
  const uint32_t *sizes;
  RegionArgs ra;
  DstDesc d;
};
__global__ __launch_bounds__(kDecThreads) void k_dec_region_p(RegionArgsP a) {
  constexpr bool kRegionTens = false, kRegionPitch = true;
  constexpr bool kRegionConceal = false, kRegionMap = false;
  uint8_t *const cmap = nullptr;
  const int32_t *const smap = nullptr;
  int32_t *const wstat = nullptr;
  const Geom &g = a.g;
  const DecWs &ws = a.ws;
  const uint8_t *packed = a.packed;
  const size_t in_stride = a.in_stride;
  const uint32_t *sizes = a.sizes;
  const RegionArgs &ra = a.ra;
  const TensK td = nullptr;
  const DstK pd = &((const __attribute__((address_space(4))) RegionArgsP *)__builtin_amdgcn_kernarg_segment_ptr())->d;
#include "dec_body_region.inc"
}

// The region decode's per-frame forms of the kernels it shares with the full decode: frame f's
// touched rows [r0_f, r1_f) come from its origin (org[2 f + 1] = y_f) and the window height h.
// The grids are sized by the batch's largest row count; a workgroup past its frame's last row
// returns before it loads anything.  Each includes the body of the full decode's kernel
// (dec_body_*.inc) behind its own per-frame values of that kernel's parameters: the full decode's
// kernels keep their code instruction for instruction, and there is one copy of each body.
__device__ __forceinline__ int region_r0(const int32_t *org, int f) { return org[2 * f + 1] / 8; }
__device__ __forceinline__ int region_r1(const int32_t *org, int f, int h) { return (org[2 * f + 1] + h + 7) / 8; }

// k_dec_rowwalk stopping at each frame's own r1_f (to the end of the chunk where r1_f is the last row).
__global__ __launch_bounds__(64) void k_region_rowwalk(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                       const uint32_t *sizes, const int32_t *org, int h) {
  const int r1_f = region_r1(org, blockIdx.x, h);
  const int row_end = r1_f == g.rows ? 0x7fffffff : r1_f, resume = 0;
#include "dec_body_rowwalk.inc"
}

// k_dec_set_index over a batch: frame f = blockIdx.x sees its own record, size, row tables and index
// (at index + 2 f rows), rows [r0_f, r1_f) filled.
__global__ __launch_bounds__(256) void k_region_set_index(Geom g, DecWs ws_all, const uint32_t *index_all,
                                                          const uint32_t *sizes_all, const int32_t *org, int h) {
  const int f_ = blockIdx.x;
  DecWs ws = ws_all;
  ws.frames += f_;
  ws.row_off += (size_t)f_ * g.rows;
  ws.row_len += (size_t)f_ * g.rows;
  const uint32_t *index = index_all + (size_t)f_ * 2 * g.rows, *sizes = sizes_all + f_;
  const int r0 = region_r0(org, f_), r1 = region_r1(org, f_, h);
#include "dec_body_set_index.inc"
}

// k_row_count<false> over each frame's own rows (rows_per_wg of them per workgroup).
__global__ __launch_bounds__(kDecThreads, 8) void k_region_count(Geom g, DecWs ws, const uint8_t *packed,
                                                                size_t in_stride, const uint32_t *sizes,
                                                                const int32_t *org, int h, int rows_per_wg) {
  constexpr bool LDSPAY = false;
  const int r0 = region_r0(org, blockIdx.y), r1 = region_r1(org, blockIdx.y, h);
  if (r0 + (int)blockIdx.x * rows_per_wg >= r1) return;
#include "dec_body_row_count.inc"
}

// k_row_count_w over each frame's own rows.
__global__ __launch_bounds__(kDecThreads, 8) void k_region_count_w(Geom g, DecWs ws, const uint8_t *packed,
                                                                  size_t in_stride, const uint32_t *sizes,
                                                                  const int32_t *org, int h) {
  const int r0 = region_r0(org, blockIdx.y), r1 = region_r1(org, blockIdx.y, h);
  if (r0 + (int)blockIdx.x * kCountRowsW >= r1) return;
  constexpr int NQ = 1;   // a sub-sequence per lane
#include "dec_body_row_count_w.inc"
}

// k_region_walk_end: k_dec_rowwalk stopped at row_end = r1 < rows flags a FRES chunk that ends right
// behind row r1 - 1 as "fewer blocks than block rows" -- a verdict on the rows from r1 on, which
// the region decode does not look at (region_index accepts such a stream).  For a frame whose parse
// passed and whose walk says so, the headers of rows 0 .. r1-1 are walked again (only those bytes):
// where they are whole and the chunk ends exactly behind row r1 - 1, the verdict is withdrawn.
// r1 = r1_f, the frame's own; a frame whose r1_f is the last row walked to the end of the chunk.
__global__ void k_region_walk_end(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride, const int32_t *org, int h,
                                  int batch) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= batch) return;
  const int r1 = region_r1(org, f, h);
  if (r1 >= g.rows) return;
  DecFrame *df = ws.frames + f;
  if (df->parse_status != 0 || df->walk_status != fmt_err(7, 1) || df->walk_q != 0) return;
  const uint8_t *p = packed + (size_t)f * in_stride;
  const uint32_t end = df->s[1].chunk_end;
  uint32_t q = df->s[1].payload_off;
  for (int r = 0; r < r1; ++r) {   // (k_dec_rowwalk's header rules; the whole chunk is present)
    uint32_t b, len, need;
    if (pfx_row_header(p, q, end, end, &b, &len, &need) != kPfxOk) return;
    q = b + len;
  }
  if (q == end) df->walk_status = 0;
}

// ---------------------------------------------------------------------------
// MANY WINDOWS OF ONE STREAM (himg_hip_decode_stream_regions_device): window k is the w x h rectangle at
// its own origin of stream s_k = stream_of[k].  The head phase and the row index are per STREAM and run once
// however many windows name a stream; the verdict is per WINDOW, exactly that of the region decode of the
// stream with that rectangle alone.  So nothing a row says reaches DecFrame::status, which keeps the head's
// verdict (RIFF .. FMAP, the FRES tree, the LRES chain) alone:
//   k_stream_rowwalk / k_stream_set_index   one walk per stream to the largest r1_k of its windows (to the
//                      end of the chunk when a window reaches the last block row).  What it found goes to
//                      words of its own, walk_rows[s] -- the rows whose headers it delimited -- and walk_st[s]
//                      -- k_dec_rowwalk's verdict of a walk to the end of the chunk --, and
//                      DecFrame::walk_status is cleared, so that the count kernels fold nothing into the frame.
//   k_stream_gate      (a lane per window) wstat[k], window k's own word, starts as the walk's verdict FOR
//                      r1_k: a window below the last block row needs rows 0 .. r1_k - 1 delimited and nothing
//                      more (k_region_walk_end's rule: a chunk that ends right behind row r1_k - 1 is
//                      accepted); one that reaches the last block row takes the verdict of the whole walk.
//   k_stream_count(_w) k_row_count<false> / k_row_count_w over a LIST of (stream, first row, last row) runs the
//                      host has deduplicated: a block row that several windows touch is counted once.
//   k_dec_stream_region   k_dec_region's body on a grid of (strip, row - r0_k, window): the records,
//                      tables and low-res plane of stream s_k, read only; a rejected row is raised into
//                      wstat[k].
//   k_stream_status    d_status[k] = max(head verdict of s_k, wstat[k]).
// ---------------------------------------------------------------------------
struct StreamWinWords {       // per launch (himg_hip.hip stages the first five, the rest is scratch)
  const int32_t *stream_of;   // [n_windows] s_k
  const int32_t *org;         // [2 n_windows] (x_k, y_k)
  const int32_t *row_end;     // [n_streams] where stream s's walk stops: 0 for a stream no window names
  const int32_t *list;        // [3 n_list] (stream, first row, end row) of a count workgroup
  const int32_t *index_rows;  // [2 n_streams] k_stream_set_index: the rows the host's index holds
  int32_t *walk_rows, *walk_st;   // [n_streams]
  int32_t *wstat;             // [n_windows]
};
constexpr int kWalkNoVerdict = 0x7fffffff;   // walk_rows: the walk has nothing to say (the parse's verdict, or one row)

__global__ __launch_bounds__(64) void k_stream_rowwalk(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                       const uint32_t *sizes, StreamWinWords sw) {
  const int row_end = sw.row_end[blockIdx.x], resume = 0;
  if (threadIdx.x == 0) {
    sw.walk_rows[blockIdx.x] = kWalkNoVerdict; sw.walk_st[blockIdx.x] = 0;
    if (row_end == 0) ws.frames[blockIdx.x].walk_status = 0;
  }
  if (row_end == 0) return;
#include "dec_body_rowwalk.inc"
  // (lane 0, behind the row headers: r rows delimited; st, the verdict where the walk reached the chunk's end)
  sw.walk_rows[f] = r; sw.walk_st[f] = st;
  df->walk_status = 0;
}

// k_region_set_index with a row range per stream; an index that points outside the stream fails every window.
__global__ __launch_bounds__(256) void k_stream_set_index(Geom g, DecWs ws_all, const uint32_t *index_all,
                                                          const uint32_t *sizes_all, StreamWinWords sw) {
  const int f_ = blockIdx.x;
  DecWs ws = ws_all;
  ws.frames += f_;
  ws.row_off += (size_t)f_ * g.rows;
  ws.row_len += (size_t)f_ * g.rows;
  const uint32_t *index = index_all + (size_t)f_ * 2 * g.rows, *sizes = sizes_all + f_;
  const int r0 = sw.index_rows[2 * f_], r1 = sw.index_rows[2 * f_ + 1];
#include "dec_body_set_index.inc"
  if (threadIdx.x == 0) {
    sw.walk_rows[f_] = bad ? 0 : kWalkNoVerdict; sw.walk_st[f_] = bad ? fmt_err(7, 1) : 0;
    df->walk_status = 0;
  }
}

__global__ void k_stream_gate(Geom g, DecWs ws, StreamWinWords sw, int h, int n_windows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_windows) return;
  const int s = sw.stream_of[k], r1 = region_r1(sw.org, k, h);
  int v = 0;
  if (ws.frames[s].parse_status == 0)   // (k_row_count's rule: the walk's verdict counts if the parse passed)
    v = r1 >= g.rows ? sw.walk_st[s] : (sw.walk_rows[s] < r1 ? fmt_err(7, 1) : 0);
  sw.wstat[k] = v;
}

// The count kernels over the list: entry e = (stream, r0, r1) is one workgroup's rows.  The bodies take the
// frame from blockIdx.y and their first row from blockIdx.x: here both are the entry's, under those names.
__global__ __launch_bounds__(kDecThreads, 8) void k_stream_count(Geom g, DecWs ws, const uint8_t *packed,
                                                                size_t in_stride, const uint32_t *sizes,
                                                                StreamWinWords sw, int rows_per_wg) {
  constexpr bool LDSPAY = false;
  const int32_t *e = sw.list + 3 * (size_t)blockIdx.x;
  const int es = __builtin_amdgcn_readfirstlane(e[0]);
  const int r0 = e[1], r1 = min(e[2], sw.walk_rows[es]);   // (rows the walk did not delimit have no index)
  if (r0 >= r1) return;
  const struct { unsigned x, y; } blockIdx = {0u, (unsigned)es};
#include "dec_body_row_count.inc"
}

__global__ __launch_bounds__(kDecThreads, 8) void k_stream_count_w(Geom g, DecWs ws, const uint8_t *packed,
                                                                  size_t in_stride, const uint32_t *sizes,
                                                                  StreamWinWords sw) {
  const int32_t *e = sw.list + 3 * (size_t)blockIdx.x;
  const int es = __builtin_amdgcn_readfirstlane(e[0]);
  const int r0 = e[1], r1 = min(e[2], sw.walk_rows[es]);
  if (r0 >= r1) return;
  const struct { unsigned x, y; } blockIdx = {0u, (unsigned)es};
  constexpr int NQ = 1;   // a sub-sequence per lane
#include "dec_body_row_count_w.inc"
}

__global__ __launch_bounds__(kDecThreads) void k_dec_stream_region(Geom g, DecWs ws, const uint8_t *packed,
                                                                  size_t in_stride, const uint32_t *sizes,
                                                                  RegionArgs ra, const int32_t *smap, int32_t *wstat) {
  constexpr bool kRegionTens = false, kRegionPitch = false;
  constexpr bool kRegionConceal = false, kRegionMap = true;
  uint8_t *const cmap = nullptr;
  const TensK td = nullptr;
  const DstK pd = nullptr;
#include "dec_body_region.inc"
}

__global__ void k_stream_status(DecWs ws, StreamWinWords sw, int32_t *status, int n_windows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_windows) return;
  const int hd = ws.frames[sw.stream_of[k]].status, own = sw.wstat[k];
  status[k] = hd > own ? hd : own;
}

// ---------------------------------------------------------------------------
// OPENED STREAMS (himg_hip_open_streams_device, himg_hip_opened_regions_device): the products of the head --
// DecFrame, the FRES tables, the row index, the low-res plane -- and the rows' records live in a HANDLE's
// buffers, behind a DecWs of their own, and outlast the call.  Open runs the head of the many-windows decode
// with these forms:
//   k_open_rowwalk / k_open_set_index   k_stream_rowwalk / k_stream_set_index over ALL rows of every stream: one
//                      walk serves whatever r1 a later window has.  walk_rows[s] and walk_st[s] are the handle's.
//   k_open_finish      clears the valid word of every row record -- an uncounted row can never be read as
//                      counted (the row kernel walks such a row serially: slow, never wrong) -- and copies the
//                      head verdicts out.
// A call on the handle runs no head:
//   k_opened_gate      k_stream_gate from the kept walk words, and the kept head verdict with it:
//                      status[k] = max(head of s_k, walk verdict for r1_k), written straight to the caller's
//                      d_status, which then serves k_dec_stream_region as its window words.  That kernel reads
//                      head | word and raises a rejected row with atomicMax: the word ends as
//                      max(head, walk, row), which is k_stream_status's max(head, max(walk, row)).
//   k_stream_count(_w) over the rows of this call's windows that no earlier call has counted (the host keeps
//                      the bitmap), into the handle's records; no launch where nothing is new.  A record's
//                      valid word is 1 (k_stream_count) or 3 (k_stream_count_w) whichever call wrote it;
//                      dec_body_region.inc asks only valid != 0 and walks a lane's range token by token to
//                      the next lane's start either way, so records of both forms serve one handle.
//   k_dec_stream_region   as it is, against the handle's DecWs.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_open_rowwalk(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                     const uint32_t *sizes, int32_t *walk_rows, int32_t *walk_st) {
  constexpr int row_end = 0x7fffffff, resume = 0;
  if (threadIdx.x == 0) { walk_rows[blockIdx.x] = kWalkNoVerdict; walk_st[blockIdx.x] = 0; }
#include "dec_body_rowwalk.inc"
  walk_rows[f] = r; walk_st[f] = st;
  df->walk_status = 0;
}

__global__ __launch_bounds__(256) void k_open_set_index(Geom g, DecWs ws_all, const uint32_t *index_all,
                                                        const uint32_t *sizes_all, int32_t *walk_rows, int32_t *walk_st) {
  const int f_ = blockIdx.x;
  DecWs ws = ws_all;
  ws.frames += f_;
  ws.row_off += (size_t)f_ * g.rows;
  ws.row_len += (size_t)f_ * g.rows;
  const uint32_t *index = index_all + (size_t)f_ * 2 * g.rows, *sizes = sizes_all + f_;
  const int r0 = 0, r1 = g.rows;
#include "dec_body_set_index.inc"
  if (threadIdx.x == 0) {
    walk_rows[f_] = bad ? 0 : kWalkNoVerdict; walk_st[f_] = bad ? fmt_err(7, 1) : 0;
    df->walk_status = 0;
  }
}

__global__ void k_open_finish(Geom g, DecWs ws, int32_t *head_status, int n_streams) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)n_streams * g.rows) ws.lane_off[i * (kDecThreads + kRecHdr) + kDecThreads + 2] = 0;
  if (head_status && i < (size_t)n_streams) head_status[i] = ws.frames[i].status;
}

__global__ void k_opened_gate(Geom g, DecWs ws, const int32_t *stream_of, const int32_t *org, const int32_t *walk_rows,
                              const int32_t *walk_st, int32_t *status, int h, int n_windows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_windows) return;
  const int s = stream_of[k], r1 = region_r1(org, k, h);
  int v = 0;
  if (ws.frames[s].parse_status == 0)   // (k_stream_gate's rule)
    v = r1 >= g.rows ? walk_st[s] : (walk_rows[s] < r1 ? fmt_err(7, 1) : 0);
  const int hd = ws.frames[s].status;
  status[k] = hd > v ? hd : v;
}

// ---------------------------------------------------------------------------
// The ROW-SPAN family: block rows [k0_f, k1_f) of frame f at the full width, k0_f and k1_f known ON THE
// DEVICE alone, so the count and row kernels take them from arrays where the region forms compute r1_f
// from an origin; like those, each includes the body of the kernel it stands beside behind its own
// values.  Rows [kfill_f, rows) are written from the low-res plane alone.  Three decodes run it
// (include/himg_hip.h):
//   * the decode of a stream PREFIX, the first avail_f bytes of frame f's stream: k0 = 0, k1 = kfill = k_f,
//     the block rows whose size header and payload lie wholly below avail_f;
//   * the prefix decode CONTINUED (himg_hip_decode_prefix_more_device): frame f comes with a PfxState in
//     device memory.  A fresh state (started == 0) makes the frame the prefix decode's, to the byte.
//     Otherwise block rows [0, k_prev) are in the caller's picture already: the head runs as it always does
//     (the workspace keeps nothing between calls), the header walk resumes where the state says, and only
//     rows [k0, k1) = [k_prev, k_new) are counted, decoded and stored; kfill = rows, so that the fill skips
//     the frame whole -- its missing rows are in the caller's picture too;
//   * the CONCEALING decode (below), whose own gate and walk set k0 = 0 and k1 = kfill = k_f.
// The kernels:
//   k_span_gate        (one wavefront per frame) the chunk headers RIFF .. FRES and the length of the
//                      FRES tree with every load checked against avail_f (prefix_walk.h).  A frame
//                      whose head has not arrived whole gets the verdict kStShort, and the size 0
//                      goes to the parse and to every reader for it: nothing of it is loaded again.
//                      For the others: tx[f] = T_f, the container's bound for k_dec_parse_prefix;
//                      bound[f] = avail_f, the load bound of every later kernel; DecFrame::walk_q /
//                      walk_end = where the row headers start and the chunk ends.  Then the frame's state,
//                      if there is one and it is started, against those results, every field before
//                      anything uses it.  A state that cannot be right: the verdict kStGeom -- the word the
//                      host maps to HIMG_ERR_ARG -- and the frame is closed like one below its head.
//                      Otherwise k0[f] = k1[f] = k_prev until the walk says more, and the walk resumes at
//                      the state's position.
//   k_span_rowwalk     (one lane per frame) the row headers below avail_f from the walk's position: the
//                      row index of rows [k0, k1), k1, where the walk stands now.
//   k_prefix_fill      rows [kfill_f, rows) from the low-res plane.
//   k_span_count(_w)   k_row_count<false> / k_row_count_w over rows [k0, k1).
//   k_dec_span         k_dec_region's body over the window (0, 8 k0, W, min(8 k1, H) - 8 k0), placed at
//                      its rows of the full picture.
//   k_span_status      the verdicts, k1 (-1 for a frame with a verdict), and the states of the frames
//                      without one.
// ---------------------------------------------------------------------------
constexpr int kStShort = 5;   // the prefix ends before the first row header: HIMG_ERR_CAPACITY

struct SpanWords {        // per-frame words of one launch (the launch function carves them)
  const uint32_t *avail;  // the bytes present, as the caller staged them
  uint32_t *tx, *bound;   // the gate's: the declared size, the load bound
  int32_t *k0, *k1;       // the rows to decode, [k0, k1)
  int32_t *gate;          // the gate's verdict
  int32_t *kfill;         // k_prefix_fill's k_f
  uint32_t *pos;          // PfxRows::used of this call's walk
};

__global__ __launch_bounds__(64) void k_span_gate(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                  const PfxState *state, SpanWords w) {
  __shared__ uint8_t s_tree[kTreeStride];
  __shared__ uint32_t s_hdr[4];
  const int f = blockIdx.x, lane = threadIdx.x;
  DecFrame *df = ws.frames + f;
  const uint8_t *p = packed + (size_t)f * in_stride;
  const uint32_t avail = w.avail[f];
  if (lane == 0) {
    PfxHead h;
    int rc = pfx_chain(p, avail, g.fix_t2, (uint32_t)g.row_block, &h);
    // A geometry other than the launch's: k_dec_parse says so (its loads end with FRMT's).
    const bool geom = h.frmt && ((int)h.W != g.W || (int)h.H != g.H || (int)h.C != g.C);
    if (geom) rc = kPfxFormat;
    if (rc == kPfxFormat && !geom && h.need > avail) rc = kPfxShort;   // an earlier check may need those bytes
    s_hdr[0] = (uint32_t)rc; s_hdr[1] = h.coff; s_hdr[2] = h.csz; s_hdr[3] = h.T;
    df->walk_status = rc == kPfxFormat ? (geom ? kStGeom : fmt_err(h.stage, h.huff)) : 0;
    df->rows_first = 0;
  }
  __syncthreads();
  int rc = (int)s_hdr[0];
  const uint32_t coff = s_hdr[1], csz = s_hdr[2], T = s_hdr[3];
  uint32_t have = 0;
  if (rc == kPfxOk) {   // the serialised tree as far as it has arrived (at most kTreeStride bytes)
    const uint32_t cnt = csz < (uint32_t)kTreeStride ? csz : (uint32_t)kTreeStride;
    have = avail > coff ? (avail - coff < cnt ? avail - coff : cnt) : 0u;
    for (uint32_t k = lane; k < have; k += 64u) s_tree[k] = p[coff + k];
  }
  __syncthreads();
  if (lane != 0) return;
  uint32_t wq = 0, wend = 0;   // the first row header and the chunk's end (0: no rows to walk)
  if (rc == kPfxOk) {
    uint32_t tb = 0;
    rc = pfx_tree_len(s_tree, have, csz, &tb);
    if (rc == kPfxFormat) {
      df->walk_status = fmt_err(7, 1);   // (k_dec_parse rejects this tree: its verdict comes first)
    } else if (rc == kPfxOk) {
      const uint32_t q = coff + tb, end = coff + csz;
      if (q < end) { df->rows_first = q; df->walk_end = end; wq = q; wend = end; }
      // (q >= end: nothing behind the tree -- k_dec_parse's verdict, huffman_dec.cpp:277-278)
    }
  }
  const bool is_short = rc == kPfxShort;
  int gt = is_short ? kStShort : 0, k0 = 0, kfill = 0;
  uint32_t tx = is_short ? 0u : T, bound = is_short ? 0u : avail, pos = 0;
  PfxState s;
  s.started = 0;
  if (state) {
    const uint4 raw = *reinterpret_cast<const uint4 *>(state + f);
    s.started = raw.x; s.rows_done = (int32_t)raw.y; s.walk_pos = raw.z; s.avail_seen = raw.w;
  }
  if (s.started) {   // (else a fresh frame: the prefix decode's)
    bool bad = avail < s.avail_seen;
    // (wq == 0: the verdict above, or the parse's -- that one stands)
    if (!bad && gt == 0 && wq != 0) bad = !pfx_state_ok(s, avail, g.rows, wq, wend);
    kfill = g.rows;
    if (bad) {
      gt = kStGeom;
      tx = 0; bound = 0;
      df->walk_status = 0; df->rows_first = 0;
      wq = 0;
    } else if (wq != 0) {
      k0 = s.rows_done;
      wq = pos = s.walk_pos;
    }
  }
  df->walk_q = wq;
  w.gate[f] = gt; w.tx[f] = tx; w.bound[f] = bound;
  w.k0[f] = k0; w.k1[f] = k0; w.kfill[f] = kfill; w.pos[f] = pos;
}

__global__ __launch_bounds__(64) void k_span_rowwalk(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                     SpanWords w, int batch) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= batch) return;
  DecFrame *df = ws.frames + f;
  const uint32_t q = df->walk_q;
  if (q == 0) return;   // no rows to walk: the gate's verdict, or the parse's
  df->walk_q = 0;
  PfxRows pr;
  const int rc = pfx_rows_from(packed + (size_t)f * in_stride, w.bound[f], w.tx[f], g.fix_t2, g.rows, q, w.k0[f],
                               df->walk_end, ws.row_off + (size_t)f * g.rows, ws.row_len + (size_t)f * g.rows, &pr);
  if (rc == kPfxFormat) { df->walk_status = fmt_err(7, 1); return; }
  w.k1[f] = pr.k;
  w.pos[f] = pr.used;
  if (w.kfill[f] != g.rows) w.kfill[f] = pr.k;   // (a fresh frame: the fill's k_f is the walk's)
}

// k_row_count<false> over rows [k0, k1) (rows_per_wg of them per workgroup).
__global__ __launch_bounds__(kDecThreads, 8) void k_span_count(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                              const uint32_t *sizes, const int32_t *k0,
                                                              const int32_t *k1, int rows_per_wg) {
  constexpr bool LDSPAY = false;
  const int r0 = k0[blockIdx.y], r1 = k1[blockIdx.y];
  if (r0 + (int)blockIdx.x * rows_per_wg >= r1) return;
#include "dec_body_row_count.inc"
}

// k_row_count_w over rows [k0, k1).
__global__ __launch_bounds__(kDecThreads, 8) void k_span_count_w(Geom g, DecWs ws, const uint8_t *packed,
                                                                size_t in_stride, const uint32_t *sizes,
                                                                const int32_t *k0, const int32_t *k1) {
  const int r0 = k0[blockIdx.y], r1 = k1[blockIdx.y];
  if (r0 + (int)blockIdx.x * kCountRowsW >= r1) return;
  constexpr int NQ = 1;   // a sub-sequence per lane
#include "dec_body_row_count_w.inc"
}

// k_dec_region's body over the window (0, 8 k0, W, min(8 k1, H) - 8 k0) of frame f, written where the full
// decode writes it: frame f's picture at out + f * H * W * C.  kConceal: kRegionConceal of the body -- a
// rejected row sets its byte of cmap and is stored as zero symbols.
struct SpanArgs {
  const int32_t *k0, *k1;   // [f] the rows to decode
  uint8_t *cmap;            // [f][rows] (kConceal)
  int sw;                   // tiles per column strip (blockIdx.x = strip)
  uint8_t *out;
};
struct SpanOrigin {       // every window starts at (0, y)
  int y;
  __device__ __forceinline__ int operator[](int i) const { return (i & 1) ? y : 0; }
};
struct SpanWindow {       // what the body reads of a RegionArgs
  SpanOrigin org;
  int sw, w, h;
  uint8_t *out;           // (the body adds f * h * w * C)
};
template <bool kConceal>
__global__ __launch_bounds__(kDecThreads) void k_dec_span(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                         const uint32_t *sizes, SpanArgs sa) {
  constexpr bool kRegionTens = false, kRegionPitch = false, kRegionConceal = kConceal, kRegionMap = false;
  uint8_t *const cmap = sa.cmap;
  const int32_t *const smap = nullptr;
  int32_t *const wstat = nullptr;
  const TensK td = nullptr;
  const DstK pd = nullptr;
  const int k0 = sa.k0[blockIdx.z], k1 = sa.k1[blockIdx.z];
  if ((int)blockIdx.y >= k1 - k0) return;
  SpanWindow ra;
  ra.org.y = 8 * k0;
  ra.sw = sa.sw; ra.w = g.W; ra.h = (8 * k1 < g.H ? 8 * k1 : g.H) - 8 * k0;
  // The body places frame f at ra.out + f * ra.h * ra.w * C (dec_body_region.inc, "img = ra.out + ...", which names
  // this kernel): with a height per frame the rest of the full picture's stride is added here, so that frame
  // f lands at sa.out + f * H * W * C -- then down to the window's first pixel row.
  ra.out = sa.out + (size_t)blockIdx.z * ((size_t)(g.H - ra.h) * g.W * g.C) + (size_t)(8 * k0) * ((size_t)g.W * g.C);
#include "dec_body_region.inc"
}

// k_prefix_fill: the block rows that have not arrived, [k_f, rows) of frame f -- what the full decode
// writes for a row whose symbols are all zero: the tile's interpolated low-res block (GetLowresBlock,
// downsampled.cpp:116-169; bytes, so the decoder's clamp changes nothing), the colour inverse
// (ycbcr.cpp:54-82) where the frame asks for it, clipped at the right and bottom edges.  It reads the
// low-res plane only (four samples per tile and channel) and is a pure store stream:
//   * a workgroup per (128 tiles, block row, frame); one whose row is below k_f returns at once;
//   * a lane per HALF tile, lane 2 t + h: columns 4 h .. 4 h + 3 of tile t, all eight pixel rows.  For
//     RGBA that is one 16-byte store per pixel row, and a wavefront's 64 stores of a pixel row are
//     1 KiB of contiguous bytes;
//   * the vertical interpolation is lowres_quads' (four rows per register), the horizontal one only
//     the half's four columns: with (lo, hi) = (left, middle) or (middle, right) they are
//     lo, lerp(lo, m), m = lerp(lo, hi), lerp(m, hi) -- interp9's tree restricted to one half;
//   * C < 4, a tile the right or bottom edge cuts, and a frame whose pixels are not 16-byte aligned
//     take the byte path.
// No LDS, no state of the row kernels.
__device__ __forceinline__ void fill_half(uint32_t l4, uint32_t r4, int hh, uint32_t x[4]) {
  const uint32_t rnd = 0x01010101u;
  const uint32_t m4 = __builtin_amdgcn_lerp(l4, r4, rnd);
  const uint32_t lo = hh ? m4 : l4, hi = hh ? r4 : m4;
  const uint32_t m = __builtin_amdgcn_lerp(lo, hi, rnd);
  x[0] = lo; x[1] = __builtin_amdgcn_lerp(lo, m, rnd); x[2] = m; x[3] = __builtin_amdgcn_lerp(m, hi, rnd);
}

__global__ __launch_bounds__(256) void k_prefix_fill(Geom g, DecWs ws, const int32_t *krows, uint8_t *out) {
  const int f = blockIdx.z, v = blockIdx.y;
  if (v < krows[f]) return;
  const DecFrame *df = ws.frames + f;
  if (df->status != 0 || (df->parse_status == 0 && df->walk_status != 0)) return;
  const int it = (int)blockIdx.x * 256 + (int)threadIdx.x, u = it >> 1, hh = it & 1;
  const int cols = g.cols, C = g.C, W = g.W, H = g.H;
  if (u >= cols) return;
  const int v2 = v + 1 < g.rows ? v + 1 : g.rows - 1, u2 = u + 1 < cols ? u + 1 : cols - 1;
  const uint8_t *low = ws.low + (size_t)f * ws.plane_stride;
  uint32_t X[4][2][4];   // [channel][q][k]: the bytes of pixel rows 4 q .. 4 q + 3 at column 4 hh + k
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c < C) {
      const uint8_t *m = low + (size_t)c * g.rows * cols;
      uint32_t lr[9];
      lr[0] = (uint32_t)m[(size_t)v * cols + u] | ((uint32_t)m[(size_t)v * cols + u2] << 8);
      lr[8] = (uint32_t)m[(size_t)v2 * cols + u] | ((uint32_t)m[(size_t)v2 * cols + u2] << 8);
      interp9_u8x4(lr);   // bytes 0, 1 = left, right of rows 0 .. 7
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint32_t p01 = __builtin_amdgcn_perm(lr[4 * q + 1], lr[4 * q], 0x05010400u);      // L0 L1 R0 R1
        const uint32_t p23 = __builtin_amdgcn_perm(lr[4 * q + 3], lr[4 * q + 2], 0x05010400u);  // L2 L3 R2 R3
        fill_half(__builtin_amdgcn_perm(p23, p01, 0x05040100u), __builtin_amdgcn_perm(p23, p01, 0x07060302u), hh,
                  X[c][q]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) X[c][q][k] = 0;
    }
  }
  const int ycc = df->ycbcr;
  const int x0 = 8 * u + 4 * hh, y0 = 8 * v;
  if (x0 >= W) return;
  uint8_t *img = out + (size_t)f * ((size_t)H * W * C);
  const bool wide = C == 4 && x0 + 4 <= W && ((((uintptr_t)img) | ((size_t)W * 4)) & 15u) == 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int y = y0 + 4 * q + i;
      if (y >= H) continue;
      uint32_t px[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t c0 = (X[0][q][k] >> (8 * i)) & 255u, c1 = (X[1][q][k] >> (8 * i)) & 255u;
        uint32_t c2 = (X[2][q][k] >> (8 * i)) & 255u;
        const uint32_t c3 = (X[3][q][k] >> (8 * i)) & 255u;
        if (ycc) ycc_to_rgb(c0, c1, c2);
        px[k] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
      }
      uint8_t *d = img + ((size_t)y * W + x0) * C;
      if (wide) {
        *reinterpret_cast<uint4 *>(d) = make_uint4(px[0], px[1], px[2], px[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (x0 + k >= W) continue;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < C) d[k * C + c] = (uint8_t)(px[k] >> (8 * c));
        }
      }
    }
  }
}

// The verdicts: k_dec_status's rule, then the gate's word for a frame it stopped, and k1.  With states, a
// frame without a verdict hands its state on: {1, k1, the walk's position, avail}.
__global__ void k_span_status(DecWs ws, SpanWords w, PfxState *state, int32_t *status, int32_t *rows_out, int batch) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= batch) return;
  const DecFrame *df = ws.frames + f;
  const int ws_ = df->parse_status == 0 ? df->walk_status : 0;
  int st = df->status > ws_ ? df->status : ws_;
  if (w.gate[f]) st = w.gate[f];
  status[f] = st;
  if (rows_out) rows_out[f] = st ? -1 : w.k1[f];
  if (state && !st)
    *reinterpret_cast<uint4 *>(state + f) = make_uint4(1u, (uint32_t)w.k1[f], w.pos[f], w.avail[f]);
}

// ---------------------------------------------------------------------------
// The CONCEALING decode (include/himg_hip.h): the full decode as it is, then a repair pass over the
// frames it rejected in their FRES rows alone.  Of such a frame the rows the header walk delimits,
// [0, k_f), are judged one by one -- an accepted row is the full decode's, a rejected one is stored as a
// row of zero symbols -- and rows [k_f, rows) are the prefix decode's fill.  Every other frame keeps
// what the full decode left.
//   k_conceal_gate     (a lane per frame) act[f]: 1 a frame to repair -- the parse passed and the verdict
//                      is the rows' (the walk's or a row kernel's); its verdict fields are cleared for the
//                      kernels below.  The span of every frame starts empty (k0 = k_f = 0).  0: accepted, 2: a head verdict -- neither is touched again: an
//                      accepted frame is PARKED (DecFrame::status = kStParked until k_conceal_status), so
//                      that the kernels shared with the other decodes, which skip a frame with a verdict,
//                      skip it too.
//   k_conceal_zero     the LRES symbols of the frames to repair, then the LRES chain over them again: a
//                      verdict of the rows may have reached a frame while its chain ran, which then
//                      stopped half way (and a chain that fails now is a head verdict after all: the
//                      rows' verdict hid it).
//   k_conceal_rowwalk  (a lane per frame) the row headers again, for the row index and k_f.
//   k_conceal_map      the row map: 1 for rows [k_f, rows) of a frame to repair, else 0.
//   k_prefix_fill, k_span_count(_w), k_dec_span<true>   the row-span family over [0, k_f), with
//                      kRegionConceal: a rejected row sets its map byte and is stored as zero symbols.
//   k_conceal_status   (a wavefront per frame) d_status, d_concealed, the caller's row map.
// ---------------------------------------------------------------------------
constexpr int kStParked = 1 << 30;

__global__ void k_conceal_gate(DecWs ws, const int32_t *st1, int32_t *k0, int32_t *krows, int32_t *act, int batch) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= batch) return;
  DecFrame *df = ws.frames + f;
  const int m = st1[f];   // k_dec_status's word: the parse's, the walk's and the row kernels' verdicts merged
  int a = 0;
  if (m != 0) a = (df->parse_status == 0 && m == fmt_err(7, 1)) ? 1 : 2;
  act[f] = a;
  k0[f] = 0;
  krows[f] = 0;
  if (a == 1) { df->status = 0; df->walk_status = 0; }
  else if (a == 0) df->status = kStParked;
}

__global__ __launch_bounds__(256) void k_conceal_zero(DecWs ws, const int32_t *act) {
  const int f = blockIdx.y;
  if (act[f] != 1) return;
  uint4 *p = reinterpret_cast<uint4 *>(ws.lres_sym + (size_t)f * ws.lres_stride);
  const uint32_t n16 = (uint32_t)(ws.lres_stride / 16);   // (the stride is a multiple of 256)
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n16; k += gridDim.x * 256u) p[k] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(64) void k_conceal_rowwalk(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                        const int32_t *act, int32_t *krows, int batch) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= batch || act[f] != 1) return;
  const DecFrame *df = ws.frames + f;
  const uint8_t *p = packed + (size_t)f * in_stride;
  const uint32_t end = df->s[1].chunk_end;
  uint32_t q = df->s[1].payload_off;
  uint32_t *ro = ws.row_off + (size_t)f * g.rows, *rl = ws.row_len + (size_t)f * g.rows;
  int r = 0;
  if (g.fix_t2 && g.rows == 1) {   // one block row without a size header
    ro[0] = q; rl[0] = end - q;
    r = 1;
  } else {
    while (q != end) {   // (k_dec_rowwalk's header rules; a failure behind the last row conceals nothing)
      uint32_t b, len, need;
      if (pfx_row_header(p, q, end, end, &b, &len, &need) != kPfxOk) break;
      if (r < g.rows) { ro[r] = b; rl[r] = len; }
      ++r;
      q = b + len;
    }
  }
  krows[f] = r < g.rows ? r : g.rows;
}

__global__ __launch_bounds__(256) void k_conceal_map(const int32_t *act, const int32_t *krows, uint8_t *cmap, int rows,
                                                     int batch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)batch * rows) return;
  const int f = (int)(i / rows), r = (int)(i - (size_t)f * rows);
  cmap[i] = (act[f] == 1 && r >= krows[f]) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_conceal_status(DecWs ws, const int32_t *st1, const int32_t *act,
                                                       const uint8_t *cmap, int rows, uint8_t *rowmap, int32_t *status,
                                                       int32_t *concealed) {
  __shared__ int s_n;
  const int f = blockIdx.x, lane = threadIdx.x;
  DecFrame *df = ws.frames + f;
  const int a = act[f];
  // A frame to repair whose LRES chain failed in the repair pass: a head verdict (the full decode's word).
  const bool head = a == 2 || (a == 1 && df->status != 0);
  if (lane == 0) s_n = 0;
  __syncthreads();
  if (!head) {
    int n = 0;
    for (int r = lane; r < rows; r += 64) {
      const uint8_t b = a == 1 ? cmap[(size_t)f * rows + r] : (uint8_t)0;
      if (rowmap) rowmap[(size_t)f * rows + r] = b;
      n += b;
    }
    if (n) atomicAdd(&s_n, n);
  }
  __syncthreads();
  if (lane != 0) return;
  if (a == 0) df->status = 0;
  else if (a == 1 && head) df->status = st1[f];
  status[f] = head ? st1[f] : 0;
  concealed[f] = head ? -1 : s_n;
}

// ---------------------------------------------------------------------------
// k_dec_scaled<S>: the decode at 1/2 scale (S = 4) and 1/4 scale (S = 2): of every tile the
// S x S lowest-sequency coefficients, the S-point inverse transform, the low-res part as the
// rounded mean of F x F boxes (F = 8 / S) of the tile's interpolated low-res block -- the
// definition is in include/himg_hip.h (himg_hip_decode_scaled_device).  The coefficient scan walks
// square shells, so what a channel needs of a block row's [C][64][cols] symbols is the channel's
// first S * S segments.  The kernel is k_dec_region's shape: a workgroup per (column strip, block
// row, frame); the LDS holds the decode tables, the row tables and C x S * S symbol segments
// (guard dword, the strip's tiles, at least four guard bytes); the write pass follows the count
// record and the same verdict:
//   * a lane whose recorded symbols hold none of the needed ones (scan position below S * S, column
//     in the strip) does not walk, one that does stops behind its last needed symbol -- unless
//     the frame's tree has a leaf the reference rejects; the lane that completes the block always
//     walks its whole range with the reference's end-of-block checks;
//   * a row without a usable record: lane 0 walks the whole row with those checks;
//   * the transform: a lane per tile, scalar int32 with the int16 stores of quantize.cpp:153-165
//     and hadamard.cpp:47-74 at their places (S * S coefficients per plane: 2 x S sums of S);
//     a lane finishes its tile's S x S pixels -- RGBA: S stores of 4 S bytes, neighbouring lanes
//     neighbouring tiles, so a wavefront's stores of an output row are 1024 (512) contiguous bytes.
// A strip holds (64 / (S * S)) x region_strip_tiles' tiles: every width up to 16384 pixels is one
// strip; wider rows take several, each walking the records again.
// ---------------------------------------------------------------------------
struct ScaledArgs {
  int sw;          // tiles per column strip (blockIdx.x = strip)
  int ow, oh;      // the output's size, ceil(W / F) x ceil(H / F)
  uint8_t *out;    // frame f's samples at out + f * oh * ow * C
};
// One frame's window in the scaled picture (scaled_tile_rows_crop).
struct ScaledCrop {
  int x, y, w, h;
};

template <int S>
__host__ __device__ inline RegionLayout scaled_layout(int C, int sw) {
  RegionLayout L;
  uint32_t o = 0;
  auto carve = [&](uint32_t bytes) { uint32_t r = o; o += (bytes + 15u) & ~15u; return r; };
  L.tab = carve((uint32_t)sizeof(LdsTables));
  L.sh = carve((uint32_t)sizeof(RegionShared));
  L.rowtab = carve(4u * kRowTabWords);
  L.seg = (((uint32_t)sw + 3u) & ~3u) + 8u;
  L.sym = carve(L.seg * (uint32_t)(S * S) * (uint32_t)C);
  L.total = o;
  return L;
}

// The layout when the whole row is one strip (ONE: every width up to 16384 pixels): a channel's
// S * S needed segments are one contiguous run of the row's symbols, so the LDS keeps them as they
// lie in the row -- per channel a guard dword, S * S * cols symbols, at least four guard bytes
// (L.seg: the channel stride) -- and a symbol's address is linear in its position.
template <int S>
__host__ __device__ inline RegionLayout scaled_layout_one(int C, int cols) {
  RegionLayout L;
  uint32_t o = 0;
  auto carve = [&](uint32_t bytes) { uint32_t r = o; o += (bytes + 15u) & ~15u; return r; };
  L.tab = carve((uint32_t)sizeof(LdsTables));
  L.sh = carve((uint32_t)sizeof(RegionShared));
  L.rowtab = carve(4u * kRowTabWords);
  L.seg = (((uint32_t)(S * S) * (uint32_t)cols + 3u) & ~3u) + 8u;
  L.sym = carve(L.seg * (uint32_t)C);
  L.total = o;
  return L;
}

// ONE: put without a division.  The channel is that of the group's LAST byte (three compares
// against the channels' first symbols), so a group that starts up to three symbols in front of a
// channel lands its first bytes on that channel's front guard; a group's bytes behind a channel's
// needed run land on the tail guard, or inside the run's padding.
template <int S>
struct ScaledWinOne {
  uint32_t base;        // LDS address of channel 0's guard dword
  uint32_t chan, need, cstride, nch;   // symbols per channel (64 cols), needed ones (S * S cols), LDS channel stride, C
  __device__ __forceinline__ void put(uint32_t op, uint32_t by) const {
    const uint32_t q = op + 3u;
    const uint32_t c = (q >= chan ? 1u : 0u) + (q >= 2u * chan ? 1u : 0u) + (q >= 3u * chan ? 1u : 0u);
    const uint32_t rel = q - c * chan;   // (position in the channel) + 3
    if (rel < need + 3u && c < nch) {   // (c == C: the last bytes of a group at the row's end, zeros)
      const uint32_t a = base + c * cstride + 1u + rel;
      const unsigned long long v = (unsigned long long)by << (8u * (a & 3u));
      lds_or32(a & ~3u, (uint32_t)v);
      lds_or32((a & ~3u) + 4u, (uint32_t)(v >> 32));
    }
  }
};

// RegionWin with only the needed segments kept: segment sj = 64 c + k of the row lives at
// LDS segment S * S * c + k when k < S * S, and nowhere otherwise.
template <int S>
struct ScaledWin {
  uint32_t base;        // LDS address of segment 0
  uint32_t cols, u0, ww, seg, nseg;   // nseg = 64 C, the ROW's segments
  __device__ __forceinline__ void put(uint32_t op, uint32_t by) const {
    if (by == 0) return;   // (zeros are the clear's)
    const uint32_t s0 = op / cols;
    const int c0 = (int)(op - s0 * cols);
#pragma unroll 1
    for (uint32_t j = 0; j < 4u; ++j) {
      const uint32_t sj = s0 + j;
      const int c = c0 - (int)(j * cols) - (int)u0;   // the group's first byte, relative to the strip
      if (c0 - (int)(j * cols) < -3 || sj >= nseg) break;
      if ((sj & 63u) < (uint32_t)(S * S) && c >= -3 && c < (int)ww) {
        const uint32_t a = base + ((sj >> 6) * (uint32_t)(S * S) + (sj & 63u)) * seg + (uint32_t)(4 + c);
        const unsigned long long v = (unsigned long long)by << (8u * (a & 3u));
        lds_or32(a & ~3u, (uint32_t)v);
        lds_or32((a & ~3u) + 4u, (uint32_t)(v >> 32));
      }
    }
  }
};

// The last symbol at or before symbol e of the row that the scaled decode reads (scan position
// below S * S, column in the strip [u0, u0 + ww)); -1: there is none.
template <int S>
__device__ __forceinline__ long long scaled_last_needed(uint32_t e, uint32_t cols, uint32_t u0, uint32_t ww) {
  uint32_t se = e / cols;
  const uint32_t ce = e - se * cols;
  if ((se & 63u) < (uint32_t)(S * S)) {
    if (ce >= u0 + ww) return (long long)se * cols + u0 + ww - 1;
    if (ce >= u0) return (long long)e;
    if (se & 63u) se -= 1u;                                   // the needed segment in front of se
    else if (se >= 64u) se = se - 64u + (uint32_t)(S * S) - 1u;
    else return -1;
  } else {
    se = (se & ~63u) + (uint32_t)(S * S) - 1u;
  }
  return (long long)se * cols + u0 + ww - 1;
}

// The S-point inverse transform of hadamard.cpp:47-74 (inputs S.. zero, every F-th output; >> 3
// and the int16 store as there).
template <int S>
__device__ __forceinline__ void iwht_short(int a[S]) {
  if (S == 4) {
    const int p = a[0] + a[1], m = a[0] - a[1], q = a[2] + a[3], n = a[2] - a[3];
    a[0] = (int)(int16_t)((p + q) >> 3);
    a[1] = (int)(int16_t)((p - q) >> 3);
    a[2] = (int)(int16_t)((m - n) >> 3);
    a[3] = (int)(int16_t)((m + n) >> 3);
  } else {
    const int p = a[0] + a[1], m = a[0] - a[1];
    a[0] = (int)(int16_t)(p >> 3);
    a[1] = (int)(int16_t)(m >> 3);
  }
}

__device__ __forceinline__ void interp9d(int a[9]) {   // downsampled.cpp:116-128
  a[4] = (a[0] + a[8] + 1) >> 1;
  a[2] = (a[0] + a[4] + 1) >> 1;
  a[6] = (a[4] + a[8] + 1) >> 1;
  a[1] = (a[0] + a[2] + 1) >> 1;
  a[3] = (a[2] + a[4] + 1) >> 1;
  a[5] = (a[4] + a[6] + 1) >> 1;
  a[7] = (a[6] + a[8] + 1) >> 1;
}

__device__ __forceinline__ void interp9pk(uint32_t a[9]) {   // interp9d on both halves of each register
  auto avg = [](uint32_t x, uint32_t y) { return ((x + y + 0x00010001u) >> 1) & 0x00ff00ffu; };
  a[4] = avg(a[0], a[8]);
  a[2] = avg(a[0], a[4]);
  a[6] = avg(a[4], a[8]);
  a[1] = avg(a[0], a[2]);
  a[3] = avg(a[2], a[4]);
  a[5] = avg(a[4], a[6]);
  a[7] = avg(a[6], a[8]);
}

// One tile at scale S / 8: sym = the tile's symbol in LDS segment 0 (segment (c, k) at
// c cstride + k sstride), the low-res corners from the frame's planes at tile (u, v), S x S samples
// per channel to (S u + X, S v + Y) of the ow x oh output, clipped.  scaled_tile_rows: the output rows
// Y0 .. Y0 + NY - 1 of the tile.
template <int S, int Y0, int NY>
__device__ __forceinline__ void scaled_tile_rows(const Geom &g, int sstride, int cstride, const uint8_t *sym, const uint8_t *low,
                                                  const int16_t *s_unmap, const uint8_t *s_shift, int ycbcr, int u,
                                                  int v, const ScaledArgs &sa, uint8_t *img) {
#include "dec_body_scaled_tile.inc"
  const int x0 = S * u;
#pragma unroll
  for (int Y = Y0; Y < Y0 + NY; ++Y) {
    const int py = S * v + Y;
    if (py >= sa.oh) break;
    const uint32_t *qr = q + (Y - Y0) * S;
    uint8_t *d = img + ((size_t)py * sa.ow + x0) * C;
    if (C == 4) {
      if (x0 + S <= sa.ow && ((uintptr_t)d & (uintptr_t)(4 * S - 1)) == 0) {
        if (S == 4) *reinterpret_cast<uint4 *>(d) = make_uint4(qr[0], qr[1], qr[2], qr[3]);
        else *reinterpret_cast<uint2 *>(d) = make_uint2(qr[0], qr[1]);
      } else {
#pragma unroll
        for (int X = 0; X < S; ++X)
          if (x0 + X < sa.ow) reinterpret_cast<uint32_t *>(d)[X] = qr[X];   // (4 ow per row: dword aligned)
      }
    } else {
#pragma unroll
      for (int X = 0; X < S; ++X) {
        if (x0 + X >= sa.ow) break;
        d[X * C] = (uint8_t)qr[X];
        if (C > 1) d[X * C + 1] = (uint8_t)(qr[X] >> 8);
        if (C > 2) d[X * C + 2] = (uint8_t)(qr[X] >> 16);
      }
    }
  }
}

// The same tile for the scaled region decode: the stores cropped to the frame's window (img = the window's
// sample (0, 0), row pitch w * C).
template <int S, int Y0, int NY>
__device__ __forceinline__ void scaled_tile_rows_crop(const Geom &g, int sstride, int cstride, const uint8_t *sym, const uint8_t *low,
                                                  const int16_t *s_unmap, const uint8_t *s_shift, int ycbcr, int u,
                                                  int v, const ScaledCrop &sa, uint8_t *img) {
#include "dec_body_scaled_tile.inc"
  const int px0 = S * u - sa.x;
#pragma unroll
  for (int Y = Y0; Y < Y0 + NY; ++Y) {
    const int py = S * v + Y - sa.y;
    if (py < 0 || py >= sa.h) continue;
    const uint32_t *qr = q + (Y - Y0) * S;
    uint8_t *d = img + ((long long)py * sa.w + px0) * C;
    if (C == 4) {
      if (px0 >= 0 && px0 + S <= sa.w && ((uintptr_t)d & (uintptr_t)(4 * S - 1)) == 0) {
        if (S == 4) *reinterpret_cast<uint4 *>(d) = make_uint4(qr[0], qr[1], qr[2], qr[3]);
        else *reinterpret_cast<uint2 *>(d) = make_uint2(qr[0], qr[1]);
      } else {
#pragma unroll
        for (int X = 0; X < S; ++X)
          if (px0 + X >= 0 && px0 + X < sa.w) reinterpret_cast<uint32_t *>(d)[X] = qr[X];   // (4 w per row: dword aligned)
      }
    } else {
#pragma unroll
      for (int X = 0; X < S; ++X) {
        if (px0 + X < 0 || px0 + X >= sa.w) continue;
        d[X * C] = (uint8_t)qr[X];
        if (C > 1) d[X * C + 1] = (uint8_t)(qr[X] >> 8);
        if (C > 2) d[X * C + 2] = (uint8_t)(qr[X] >> 16);
      }
    }
  }
}

// S = 4: the tile in two halves of two output rows, each gathering and transforming the tile again
// (sixteen symbols per plane) -- one pass keeps 16 + 16 + 16 values live beside the low-res block and
// does not fit the 64 registers that let two workgroups share a CU.
template <int S>
__device__ __forceinline__ void scaled_tile_store(const Geom &g, int sstride, int cstride, const uint8_t *sym, const uint8_t *low,
                                                  const int16_t *s_unmap, const uint8_t *s_shift, int ycbcr, int u,
                                                  int v, const ScaledArgs &sa, uint8_t *img) {
  if (S == 4) {
    scaled_tile_rows<S, 0, S / 2>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
    asm volatile("" ::: "memory");   // (the second half reads the symbols again)
    scaled_tile_rows<S, S / 2, S / 2>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
  } else {
    scaled_tile_rows<S, 0, S>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
  }
}

template <int S>
__device__ __forceinline__ void scaled_tile_store_crop(const Geom &g, int sstride, int cstride, const uint8_t *sym,
                                                       const uint8_t *low, const int16_t *s_unmap, const uint8_t *s_shift,
                                                       int ycbcr, int u, int v, const ScaledCrop &sa, uint8_t *img) {
  if (S == 4) {
    scaled_tile_rows_crop<S, 0, S / 2>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
    asm volatile("" ::: "memory");   // (the second half reads the symbols again)
    scaled_tile_rows_crop<S, S / 2, S / 2>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
  } else {
    scaled_tile_rows_crop<S, 0, S>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
  }
}

// The pyramid forms' share of one tile (k_dec_row_fused_m, k_tile_inv_m): PART 0 its 4 x 4 at 1/2
// scale, PART 1 its 2 x 2 at 1/4 scale, to frame f of `level` (batch x ceil(H / F) x ceil(W / F) x C
// bytes).  scaled_tile_rows, whatever holds the symbols.
template <int PART>
__device__ __forceinline__ void pyr_tile_part(const Geom &g, int sstride, int cstride, const uint8_t *sym,
                                              const uint8_t *low, const int16_t *s_unmap, const uint8_t *s_shift,
                                              int ycbcr, int u, int v, int f, uint8_t *level) {
  constexpr int F = PART == 1 ? 4 : 2;
  ScaledArgs sa;
  sa.sw = 0; sa.ow = (g.W + F - 1) / F; sa.oh = (g.H + F - 1) / F; sa.out = level;
  uint8_t *img = level + (size_t)f * ((size_t)sa.oh * sa.ow * g.C);
  if (PART == 0) scaled_tile_rows<4, 0, 4>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
  else scaled_tile_rows<2, 0, 2>(g, sstride, cstride, sym, low, s_unmap, s_shift, ycbcr, u, v, sa, img);
}

// k_tile_inv_m: k_tile_inv in its pyramid form (PyrDesc; rows too wide for the LDS).  Level 0 is
// k_tile_inv's store where it is wanted; then the tile's two lanes share the smaller levels, read from
// the same symbols in HBM ([C][64][cols] per block row): the first lane of a pair (lanes 0..31 of a
// wavefront, neighbouring lanes neighbouring tiles) the 1/2-scale samples, the second the 1/4-scale ones.
// The arguments in one struct, as in k_tile_inv_t.
struct TileArgsM {
  Geom g;
  DecWs ws;
  int v0;
  PyrDesc m;
};
template <bool FAST>
__global__ __launch_bounds__(256) void k_tile_inv_m(TileArgsM a) {
  const Geom &g = a.g;
  const DecWs &ws = a.ws;
  const int v0 = a.v0;
  const PyrK pm = &((const __attribute__((address_space(4))) TileArgsM *)__builtin_amdgcn_kernarg_segment_ptr())->m;
#include "dec_body_tile_inv.inc"
  const int u = pair_tile(it);
  const uint8_t *sym = ws.fres_sym + (size_t)f * ws.fres_stride + (size_t)v * g.row_block;
  const uint8_t *low = ws.low + (size_t)f * ws.plane_stride;
  const int ycbcr = df->ycbcr;
  uint8_t *const l0 = pm->level[0];
  if (l0)
    transform_store_pair<(FAST ? -1 : 0), FAST>(g, g.cols, sym, low, s_unmap, &s_shift[0][0], s_shiftp, ycbcr, u,
                                                pair_half(it), v, l0 + (size_t)f * ((size_t)g.W * g.H * g.C));
  uint8_t *const l1 = pm->level[1], *const l2 = pm->level[2];
  if (pair_half(it) == 0) {
    if (l1) pyr_tile_part<0>(g, g.cols, 64 * g.cols, sym + u, low, s_unmap, &s_shift[0][0], ycbcr, u, v, f, l1);
  } else if (l2) {
    pyr_tile_part<1>(g, g.cols, 64 * g.cols, sym + u, low, s_unmap, &s_shift[0][0], ycbcr, u, v, f, l2);
  }
}

template <int S, bool ONE>
__global__ __launch_bounds__(kDecThreads, 8) void k_dec_scaled(Geom g, DecWs ws, const uint8_t *packed, size_t in_stride,
                                                           const uint32_t *sizes, ScaledArgs sa) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const RegionLayout L = ONE ? scaled_layout_one<S>(g.C, g.cols) : scaled_layout<S>(g.C, sa.sw);
  LdsTables &T = *reinterpret_cast<LdsTables *>(smem + L.tab);
  RegionShared *sh = reinterpret_cast<RegionShared *>(smem + L.sh);
  const int16_t *s_unmap = reinterpret_cast<const int16_t *>(smem + L.rowtab);   // unmap, shift: contiguous
  const uint8_t *s_shift = smem + L.rowtab + 512;
  uint8_t *sym = smem + L.sym;
  const int tid = threadIdx.x, f = blockIdx.z, r = blockIdx.y;
  const int su0 = (int)blockIdx.x * sa.sw;
  if (su0 >= g.cols) return;
  const int ww = min(sa.sw, g.cols - su0);
  DecFrame *df = ws.frames + f;
  if (tid == 0) { sh->flag = df->status; sh->err = 0; sh->endbit = ~0ull; }
  __syncthreads();
  if (sh->flag) return;
  load_dec_tables(ws, df, f, 1, &T);
  if (tid < kRowTabWords / 4)
    reinterpret_cast<uint4 *>(smem + L.rowtab)[tid] = reinterpret_cast<const uint4 *>(df->row_tabs)[tid];
  const uint32_t nsym16 = (L.seg * (ONE ? 1u : (uint32_t)(S * S)) * (uint32_t)g.C + 15u) / 16u;
  for (uint32_t k = tid; k < nsym16; k += kDecThreads) reinterpret_cast<uint4 *>(sym)[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  // A tree with a leaf past the last run symbol: a walk may fail anywhere (every lane walks).
  const int nn = min(df->s[1].num_nodes, kMaxNodes + 1);
  const uint32_t nd = tid < nn ? T.nd[tid] : 0u;
  const bool strict = __syncthreads_or((nn <= 1) || ((nd >> 20) != 0 && (nd >> 20) - 1u > 260u)) != 0;

  const size_t ri = (size_t)f * g.rows + (size_t)r;
  const uint32_t pay_off = ws.row_off[ri], pay_len = ws.row_len[ri], out_size = (uint32_t)g.row_block;
  const uint8_t *p = packed + (size_t)f * in_stride;
  const uint32_t end = (uint32_t)min((unsigned long long)sizes[f], (unsigned long long)pay_off + pay_len);
  const GrpTables tb = tables_of(&T);
  typename std::conditional<ONE, ScaledWinOne<S>, ScaledWin<S>>::type win;
  if constexpr (ONE) {
    win.base = lds_addr(sym); win.chan = 64u * (uint32_t)g.cols; win.need = (uint32_t)(S * S) * (uint32_t)g.cols;
    win.cstride = L.seg; win.nch = (uint32_t)g.C;
  } else {
    win.base = lds_addr(sym); win.cols = (uint32_t)g.cols; win.u0 = (uint32_t)su0; win.ww = (uint32_t)ww;
    win.seg = L.seg; win.nseg = 64u * (uint32_t)g.C;
  }
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
        // The lane's last needed symbol (stop), if its symbols [off, off + cnt) hold one.
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
    if (tid == 0) atomicMax(&df->status, fmt_err(7, 1));
    return;
  }
  // ---- the strip's tiles: a lane per tile ----
  const uint8_t *low = ws.low + (size_t)f * ws.plane_stride;
  uint8_t *img = sa.out + (size_t)f * ((size_t)sa.oh * sa.ow * g.C);
  const int ycbcr = df->ycbcr;
#pragma unroll 1
  for (int ul = tid; ul < ww; ul += kDecThreads)
    scaled_tile_store<S>(g, ONE ? g.cols : (int)L.seg, ONE ? (int)L.seg : S * S * (int)L.seg, sym + 4 + ul, low, s_unmap,
                         s_shift, ycbcr, su0 + ul, r, sa, img);
}

// ---------------------------------------------------------------------------
// k_dec_scaled_region<S>: the window w x h of the 1/2-scale (S = 4) or 1/4-scale (S = 2) picture
// at frame f's own origin -- k_dec_scaled<S, false> over the block rows and tile columns a
// window touches, as k_dec_region is to the full decode.  The origins are those of the full-resolution
// rectangle the window covers, (F x_f, F y_f) with F = 8 / S: the region walk and count kernels
// read the same array with the height F h, and touch exactly the window's block rows
// r0_f = y_f / S .. r1_f = ceil((y_f + h) / S) (<= rows, because y_f + h <= ceil(H / F)).
// A workgroup per (column strip of sw tiles from u0_f = x_f / S on, touched block row, frame); one
// past its frame's last row or last tile returns first thing.  LDS: scaled_layout<S> -- C x S * S
// segments of the strip's tiles.  The write pass is k_dec_scaled's with ScaledWin<S> bounded to
// the window's tile columns: a lane whose recorded symbols hold no needed symbol of the window
// does not walk, one that does stops behind its last (both off under the `strict` tree rule); the
// completing lane and the no-record fallback walk the whole range with the reference's checks.
// The transform is scaled_tile_rows' (the same included body), a lane per tile, its stores cropped to the window.
// ---------------------------------------------------------------------------
struct ScaledRegionArgs {
  const int32_t *org;  // frame f's origin in full-resolution pixels (F x_f, F y_f) at org[2 f], org[2 f + 1]
  int sw;              // tiles per column strip (blockIdx.x = strip, from u0_f on)
  int w, h;            // the window, in samples of the scaled picture
  uint8_t *out;        // frame f's samples at out + f * h * w * C
};

template <int S>
__global__ __launch_bounds__(kDecThreads, 8) void k_dec_scaled_region(Geom g, DecWs ws, const uint8_t *packed,
                                                                     size_t in_stride, const uint32_t *sizes,
                                                                     ScaledRegionArgs sa) {
  constexpr bool kScaledMap = false;
  const int32_t *const smap = nullptr;
  int32_t *const wstat = nullptr;
#include "dec_body_scaled_region.inc"
}

// ---------------------------------------------------------------------------
// OPENED STREAMS, SCALED (himg_hip_opened_scaled_regions_device): window k of the picture of stream s_k at
// 1/2, 1/4 or 1/8 scale, from the handle's kept products and records and nothing else.
//   k_dec_opened_scaled_region<S>   k_dec_scaled_region<S>'s body on a grid of (strip, row - r0_k, window)
//                      under k_opened_gate, as k_dec_stream_region is k_dec_region's: the frame, records,
//                      tables and low-res plane of stream s_k, read only -- the handle's DecFrame is kept
//                      state --; the kernel reads head | wstat[k] and raises a rejected row into wstat[k], the
//                      caller's d_status word the gate has set from R^'s rows (origin (F x, F y), height F h).
//                      The records are those of the full-resolution windows: a row counted by either serves both.
//   k_opened_preview_region   the 1/8 level: k_lres_preview's arithmetic over the w x h window of stream s_k's
//                      kept plane, a lane per pixel.  The status word is the kept head verdict alone; no row is
//                      touched and the packed streams are not read.
// ---------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(kDecThreads, 8) void k_dec_opened_scaled_region(Geom g, DecWs ws, const uint8_t *packed,
                                                                            size_t in_stride, const uint32_t *sizes,
                                                                            ScaledRegionArgs sa, const int32_t *smap,
                                                                            int32_t *wstat) {
  constexpr bool kScaledMap = true;
#include "dec_body_scaled_region.inc"
}

struct PreviewWinArgs {
  const int32_t *stream_of;   // [n_windows] s_k
  const int32_t *org;         // [2 n_windows] (x_k, y_k) in the ceil(W / 8) x ceil(H / 8) picture
  int w, h;
  uint8_t *out;               // window k's pixels at out + k * h * w * C
  int32_t *status;            // [n_windows]
};

__global__ __launch_bounds__(256) void k_opened_preview_region(Geom g, DecWs ws, PreviewWinArgs pa) {
  const int k = blockIdx.y, s = __builtin_amdgcn_readfirstlane(pa.stream_of[k]);
  const DecFrame *df = ws.frames + s;
  const int hd = df->status;
  if (blockIdx.x == 0 && threadIdx.x == 0) pa.status[k] = hd;
  if (hd) return;
  const uint32_t n = (uint32_t)pa.w * (uint32_t)pa.h, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t y = i / (uint32_t)pa.w, x = i - y * (uint32_t)pa.w;
  const uint32_t npix = (uint32_t)g.rows * (uint32_t)g.cols;
  const uint32_t p = ((uint32_t)pa.org[2 * k + 1] + y) * (uint32_t)g.cols + (uint32_t)pa.org[2 * k] + x;
  const int C = g.C;
  const uint8_t *plane = ws.low + (size_t)s * ws.plane_stride;
  uint32_t v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = c < C ? plane[(size_t)c * npix + p] : 0u;
  if (df->ycbcr) ycc_to_rgb(v[0], v[1], v[2]);
  uint8_t *dst = pa.out + ((size_t)k * n + i) * (size_t)C;
  if (C == 4 && ((uintptr_t)dst & 3u) == 0) {
    *reinterpret_cast<uint32_t *>(dst) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < C) dst[c] = (uint8_t)v[c];
}

#define HIMG_LAUNCH(name, grid, block, ...)                    \
  do {                                                         \
    prof_begin(prof, #name, stream);                           \
    hipLaunchKernelGGL(name, grid, block, 0, stream, __VA_ARGS__); \
    prof_end(prof, stream);                                    \
  } while (0)

int loop_counts_read_dec(unsigned long long *out) { return loop_counts_read(out); }

// The fused row kernel's LDS budget (the whole LDS of a CU), and k_row_window's fixed need.
constexpr uint32_t kLdsMax = 160u * 1024u;
constexpr uint32_t kRowWindowLds = (uint32_t)sizeof(LdsTables) + 64u + kRowWindow + 2u * kWinGuard + 16u;

bool dec_rows_fit_lds(const Geom &g) { return fused_layout(g.row_block).total <= kLdsMax; }

// The kernels that take dynamic LDS beyond the 64 KiB a kernel gets unasked.  fixed_lds: the size it is
// allowed; 0: the whole LDS less the kernel's static share, which counts against the same 160 KiB.
hipError_t dec_set_kernel_attrs() {
#define HIMG_K(...) reinterpret_cast<const void *>(&__VA_ARGS__)
  static const struct { const void *fn; uint32_t fixed_lds; } kDynLds[] = {
      {HIMG_K(k_dec_row_fused<512>), 0},   {HIMG_K(k_dec_row_fused<256>), 0},   {HIMG_K(k_dec_row_fused<240>), 0},
      {HIMG_K(k_dec_row_fused<-1>), 0},    {HIMG_K(k_dec_row_fused<0>), 0},
      {HIMG_K(k_dec_row_fused_t<512>), 0}, {HIMG_K(k_dec_row_fused_t<-1>), 0},  {HIMG_K(k_dec_row_fused_t<0>), 0},
      {HIMG_K(k_dec_row_fused_p<512>), 0}, {HIMG_K(k_dec_row_fused_p<-1>), 0},  {HIMG_K(k_dec_row_fused_p<0>), 0},
      {HIMG_K(k_dec_row_fused_m<512>), 0}, {HIMG_K(k_dec_row_fused_m<-1>), 0},  {HIMG_K(k_dec_row_fused_m<0>), 0},
      {HIMG_K(k_dec_row_fused_c<512>), 0}, {HIMG_K(k_dec_row_fused_c<-1>), 0},  {HIMG_K(k_dec_row_fused_c<0>), 0},
      {HIMG_K(k_row_window), kRowWindowLds},
      {HIMG_K(k_dec_region), 0},           {HIMG_K(k_dec_region_t), 0},         {HIMG_K(k_dec_region_p), 0},
      {HIMG_K(k_dec_span<false>), 0},      {HIMG_K(k_dec_span<true>), 0},       {HIMG_K(k_dec_stream_region), 0},
      {HIMG_K(k_dec_scaled<4, true>), 0},  {HIMG_K(k_dec_scaled<2, true>), 0},  {HIMG_K(k_dec_scaled<4, false>), 0},
      {HIMG_K(k_dec_scaled<2, false>), 0}, {HIMG_K(k_dec_scaled_region<4>), 0}, {HIMG_K(k_dec_scaled_region<2>), 0},
      {HIMG_K(k_dec_opened_scaled_region<4>), 0}, {HIMG_K(k_dec_opened_scaled_region<2>), 0}};
#undef HIMG_K
  for (const auto &k : kDynLds) {
    uint32_t lds = k.fixed_lds;
    if (!lds) {
      hipFuncAttributes fa;
      if (hipError_t e = hipFuncGetAttributes(&fa, k.fn)) return e;
      lds = kLdsMax - (uint32_t)fa.sharedSizeBytes;
    }
    if (hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  }
  return hipSuccess;
}

int region_strip_tiles(const Geom &g) {
  const uint32_t fixed = region_layout(g.C, 0).total - region_layout(g.C, 0).seg * 64u * (uint32_t)g.C;
  const uint32_t seg = (kLdsMax - 1024u - fixed) / (64u * (uint32_t)g.C) & ~3u;   // (room for the kernel's static LDS)
  return (int)(seg - 8u);
}

int scaled_strip_tiles(const Geom &g, int scale_log2) {
  const uint32_t nseg = (scale_log2 == 1 ? 16u : 4u) * (uint32_t)g.C;
  const RegionLayout L0 = scale_log2 == 1 ? scaled_layout<4>(g.C, 0) : scaled_layout<2>(g.C, 0);
  const uint32_t fixed = L0.total - L0.seg * nseg;
  const uint32_t seg = (kLdsMax - 1024u - fixed) / nseg & ~3u;   // (room for the kernel's static LDS)
  return (int)(seg - 8u);
}

void launch_rowwalk_only(const Geom &g, const DecWs &ws, const uint8_t *d_packed, size_t in_stride,
                         const uint32_t *d_sizes, hipStream_t stream) {
  hipLaunchKernelGGL(k_dec_rowwalk, dim3(1), dim3(64), 0, stream, g, ws, d_packed, in_stride, d_sizes, 0x7fffffff, 0);
}

void launch_rowwalk_range(const Geom &g, const DecWs &ws, const uint8_t *d_packed, size_t in_stride,
                          const uint32_t *d_sizes, int row_end, bool resume, hipStream_t stream) {
  hipLaunchKernelGGL(k_dec_rowwalk, dim3(1), dim3(64), 0, stream, g, ws, d_packed, in_stride, d_sizes, row_end, resume ? 1 : 0);
}

// LRES: every chunk in parallel, chain verified, serial fallback if not; then the predictor
// inverse into the low-res plane.  d_sizes bounds the readers (the full decode: the packed
// sizes; the preview: where the LRES chunk ends).
static void launch_lres_chain(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                              const uint32_t *d_sizes, hipStream_t stream, Profiler *prof) {
  HIMG_LAUNCH(k_lres_spec, dim3(ws.lres_chunks, batch), dim3(kDecThreads), g, ws, d_packed, in_stride, d_sizes);
  HIMG_LAUNCH(k_lres_fix, dim3(batch), dim3(kDecThreads), g, ws, d_packed, in_stride, d_sizes);
  HIMG_LAUNCH(k_lres_write, dim3(ws.lres_chunks, batch), dim3(kDecThreads), g, ws, d_packed,
              in_stride, d_sizes);
  HIMG_LAUNCH(k_lres_finish, dim3((batch + 63) / 64), dim3(64), ws, batch);
  HIMG_LAUNCH(k_lres_unpredict, dim3((g.mcols + 4 * kUnpredWaves - 1) / (4 * kUnpredWaves), g.mrows, batch * g.C),
              dim3(64 * kUnpredWaves), g, ws);
}

// In front of every head phase: the diagnostics (the row counts' where the workspace has them) and the
// LRES symbols (k_lres_write stores the non-zero ones only) are cleared.
static void launch_zero(const Geom &g, const DecWs &ws, int batch, hipStream_t stream, Profiler *prof) {
  const uint32_t n16 = (uint32_t)(((size_t)batch * ws.lres_stride + 15) / 16);   // (the stride is a multiple of 256)
  const uint32_t ns = (uint32_t)((size_t)batch * (g.rows + 1) * 8), nr = ws.rc_stats ? (uint32_t)((size_t)batch * g.rows * 8) : 0u;
  prof_begin(prof, "memset", stream);
  hipLaunchKernelGGL(k_dec_zero, dim3((n16 + 256 * 4 - 1) / (256 * 4)), dim3(256), 0, stream,
                     reinterpret_cast<uint4 *>(ws.lres_sym), n16, ws.stats, ns, ws.rc_stats, nr);
  prof_end(prof, stream);
}

// The count kernel of a launch over all_rows block rows.  wave: one wavefront per row (k_row_count_w) --
// from 8192 rows per call, below that the 1024-lane kernel keeps the GPU busier (HIMG_OPT_COUNT_WAVE
// forces either); rpc: rows per workgroup of the 1024-lane kernel, which loads the decode tables once
// for its rows -- a single frame has too few rows to fill the CUs that way.  g: the geometry the count
// kernel takes.  one_record (the region and scaled decodes, whose row kernels have no parallel path for
// a row in chunks): no limit on a lane's share of the row (max_sub; the full decode splits longer rows),
// so that every row gets one record -- the lanes' ranges are 32-bit bit positions: any row a stream holds.
struct CountRule { bool wave; int rpc; Geom g; };
static CountRule count_rule(const Geom &g, long long all_rows, bool one_record) {
  CountRule c = {g.count_wave >= 0 ? g.count_wave != 0 : all_rows >= 8192,
                 all_rows <= 512 ? 1 : all_rows <= 1024 ? 2 : kRowsPerCount, g};
  if (one_record) c.g.max_sub = 0x7fffffff;
  return c;
}
// k_row_count_w over rows [a, b) of every frame, in the form the context asks for (HIMG_OPT_COUNT_STRETCH).
static void launch_row_count_w(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                               const uint32_t *d_sizes, int a, int b, hipStream_t s) {
  const dim3 grid((b - a + kCountRowsW - 1) / kCountRowsW, batch), block(kDecThreads);
  const int nq = g.count_stretch < 0 ? kCountStretch : g.count_stretch;
#define HIMG_COUNT_WN(NQ_) hipLaunchKernelGGL(k_row_count_wn<NQ_>, grid, block, 0, s, g, ws, d_packed, in_stride, d_sizes, a, b)
  if (nq == kCountStretch) hipLaunchKernelGGL(k_row_count_w, grid, block, 0, s, g, ws, d_packed, in_stride, d_sizes, a, b);
  else if (nq == 2) HIMG_COUNT_WN(2);
  else if (nq == 4) HIMG_COUNT_WN(4);
  else if (nq == 8) HIMG_COUNT_WN(8);
  else HIMG_COUNT_WN(1);
#undef HIMG_COUNT_WN
}

void launch_preview(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                    const uint32_t *d_sizes, uint32_t *d_head_sizes, uint8_t *d_out, int32_t *d_status,
                    hipStream_t stream, Profiler *prof) {
  launch_zero(g, ws, batch, stream, prof);
  HIMG_LAUNCH(k_dec_parse_head, dim3(batch), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes, d_head_sizes);
  launch_lres_chain(g, ws, batch, d_packed, in_stride, d_head_sizes, stream, prof);
  const uint32_t npix = (uint32_t)g.rows * (uint32_t)g.cols;
  HIMG_LAUNCH(k_lres_preview, dim3((npix + 1023u) / 1024u, batch), dim3(256), g, ws, d_out);
  HIMG_LAUNCH(k_dec_status, dim3((batch + 63) / 64), dim3(64), ws, d_status, batch);
}

// The batch's largest touched-row and tile-column counts (the grids; for a fixed w x h a frame's counts
// are within one of these), its touched rows (the count kernels' rule) and whether a frame's walk stops
// before the last row.  h_org: full-resolution origins; w x h: the window in the picture whose tiles are
// S x S (8, or 4 and 2 at 1/2 and 1/4 scale).
struct WindowExtents { int nrows = 0, ntiles = 0; long long all_rows = 0; bool stop_early = false; };
static WindowExtents window_extents(const Geom &g, int batch, const int32_t *h_org, int S, int w, int h) {
  WindowExtents e;
  const int F = 8 / S;
  for (int f = 0; f < batch; ++f) {
    const int x = h_org[2 * f] / F, y = h_org[2 * f + 1] / F;
    const int r0 = y / S, r1 = (y + h + S - 1) / S, nt = (x + w + S - 1) / S - x / S;
    e.nrows = r1 - r0 > e.nrows ? r1 - r0 : e.nrows;
    e.ntiles = nt > e.ntiles ? nt : e.ntiles;
    e.stop_early |= r1 < g.rows;
    e.all_rows += r1 - r0;
  }
  return e;
}

// The fork to the side stream for a header walk that runs beside the head phase on `stream` (no side streams:
// the walk runs on `stream` itself), and the join: side_walked behind the walk's launch, side_join where the
// work on `stream` first needs what it wrote.
static hipStream_t side_fork(const DecStreams *ds, hipStream_t stream) {
  if (!ds) return stream;
  (void)hipEventRecord(ds->ev_fork, stream);
  (void)hipStreamWaitEvent(ds->side, ds->ev_fork, 0);
  return ds->side;
}
static void side_walked(const DecStreams *ds) {
  if (ds) (void)hipEventRecord(ds->ev_walk[0], ds->side);
}
static void side_join(const DecStreams *ds, hipStream_t stream) {
  if (ds) (void)hipStreamWaitEvent(stream, ds->ev_walk[0], 0);
}

// scale_log2 = 0: the region decode.  1, 2: the window w x h of the picture at scale 2^-scale_log2, frame
// f's origin (x_f, y_f) in that picture; h_org / d_org hold the origins of the full-resolution rectangles
// the windows cover, (F x_f, F y_f): with the height F h the walk and count kernels, which derive a
// frame's rows on the device from d_org and that height, touch rows y_f / S .. ceil((y_f + h) / S), which
// stays within the frame's block rows because y_f + h <= ceil(H / F) (checked by the caller).
void launch_region(const Geom &g, const DecWs &ws_in, int batch, const uint8_t *d_packed, size_t in_stride,
                   const uint32_t *d_sizes, const uint32_t *d_row_index, const int32_t *h_org, const int32_t *d_org,
                   int scale_log2, int w, int h, uint8_t *d_out, int32_t *d_status, hipStream_t stream, Profiler *prof,
                   const DecStreams *ds, const StoreForm &form) {
  DecWs ws = ws_in;
  ws.lane_q = nullptr;   // (plain per-lane records: no quarter records for k_region_count)
  const int F = 1 << scale_log2, hf = F * h;
  const WindowExtents e = window_extents(g, batch, h_org, 8 / F, w, h);
  launch_zero(g, ws, batch, stream, prof);
  // Each frame's row headers up to its r1_f (all of them for the whole frame's last row: the full decode's
  // verdict), on the side stream beside k_dec_parse and the LRES chain where there is one (launch_decode's
  // fork: the serial walk to a row deep in a 16384^2 frame is as long as the LRES chain).
  hipStream_t ws_ = side_fork(ds, stream);
  prof_begin(prof, d_row_index ? "k_region_set_index" : "k_region_rowwalk", ws_);
  if (d_row_index)
    hipLaunchKernelGGL(k_region_set_index, dim3(batch), dim3(256), 0, ws_, g, ws, d_row_index, d_sizes, d_org, hf);
  else
    hipLaunchKernelGGL(k_region_rowwalk, dim3(batch), dim3(64), 0, ws_, g, ws, d_packed, in_stride, d_sizes, d_org, hf);
  prof_end(prof, ws_);
  side_walked(ds);
  HIMG_LAUNCH(k_dec_parse, dim3(batch), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes);
  launch_lres_chain(g, ws, batch, d_packed, in_stride, d_sizes, stream, prof);
  side_join(ds, stream);
  if (!d_row_index && e.stop_early)
    HIMG_LAUNCH(k_region_walk_end, dim3((batch + 63) / 64), dim3(64), g, ws, d_packed, in_stride, d_org, hf, batch);
  // Every touched row gets a record: the count kernels that read the payload in place (k_row_count<true>
  // gives up on rows beyond its LDS staging buffer, 36 KiB -- a 4096-pixel row above q50).
  const CountRule cr = count_rule(g, e.all_rows, true);
  if (cr.wave) {
    HIMG_LAUNCH(k_region_count_w, dim3((e.nrows + kCountRowsW - 1) / kCountRowsW, batch), dim3(kDecThreads), cr.g, ws,
                d_packed, in_stride, d_sizes, d_org, hf);
  } else {
    HIMG_LAUNCH(k_region_count, dim3((e.nrows + cr.rpc - 1) / cr.rpc, batch), dim3(kDecThreads), cr.g, ws, d_packed,
                in_stride, d_sizes, d_org, hf, cr.rpc);
  }
  // The row kernel over the touched block rows and tile columns, in strips of equal width.
  const int smax = scale_log2 ? scaled_strip_tiles(g, scale_log2) : region_strip_tiles(g);
  const int nstrip = (e.ntiles + smax - 1) / smax, sw = (e.ntiles + nstrip - 1) / nstrip;
  const dim3 grid(nstrip, e.nrows, batch);
  if (!scale_log2) {
    RegionArgs ra;
    ra.org = d_org; ra.sw = sw; ra.w = w; ra.h = h; ra.out = d_out;
    const dim3 block(kDecThreads);
    const uint32_t lds = region_layout(g.C, sw).total;
    if (form.kind == kStorePitch) {
      const RegionArgsP rp = {g, ws, d_packed, in_stride, d_sizes, ra, form.dst()};
      prof_begin(prof, "k_dec_region_p", stream);
      hipLaunchKernelGGL(k_dec_region_p, grid, block, lds, stream, rp);
    } else if (form.kind == kStoreTens) {
      const RegionArgsT rt = {g, ws, d_packed, in_stride, d_sizes, ra, form.tens()};
      prof_begin(prof, "k_dec_region_t", stream);
      hipLaunchKernelGGL(k_dec_region_t, grid, block, lds, stream, rt);
    } else {
      prof_begin(prof, "k_dec_region", stream);
      hipLaunchKernelGGL(k_dec_region, grid, block, lds, stream, g, ws, d_packed, in_stride, d_sizes, ra);
    }
  } else {
    ScaledRegionArgs sa;
    sa.org = d_org; sa.sw = sw; sa.w = w; sa.h = h; sa.out = d_out;
    prof_begin(prof, "k_dec_scaled_region", stream);
    if (scale_log2 == 1)
      hipLaunchKernelGGL(k_dec_scaled_region<4>, grid, dim3(kDecThreads), scaled_layout<4>(g.C, sw).total, stream, g, ws,
                         d_packed, in_stride, d_sizes, sa);
    else
      hipLaunchKernelGGL(k_dec_scaled_region<2>, grid, dim3(kDecThreads), scaled_layout<2>(g.C, sw).total, stream, g, ws,
                         d_packed, in_stride, d_sizes, sa);
  }
  prof_end(prof, stream);
  HIMG_LAUNCH(k_dec_status, dim3((batch + 63) / 64), dim3(64), ws, d_status, batch);
}

// Many windows of one stream (the kernels' comment above): the head phase over the n_streams streams as
// launch_region runs it, one walk per stream beside it, then the gate, the counts over the host's list and
// the row kernel over the windows.  d_words: the staged words and the scratch behind them, carved by the
// caller (himg_hip.hip, stream_regions_launch); list_rows: the rows the list holds, list_chunk: the most
// rows of an entry (stream_count_chunk's); d_row_index: the host's index, 2 x rows words per stream.
int stream_count_chunk(const Geom &g, long long list_rows) {
  const CountRule cr = count_rule(g, list_rows, true);
  return cr.wave ? kCountRowsW : cr.rpc;
}

void launch_stream_regions(const Geom &g, const DecWs &ws_in, int n_streams, const uint8_t *d_packed, size_t in_stride,
                           const uint32_t *d_sizes, const uint32_t *d_row_index, const StreamRegionWords &d_words,
                           int n_windows, const int32_t *h_org, int n_list, long long list_rows, int w, int h,
                           uint8_t *d_out, int32_t *d_status, hipStream_t stream, Profiler *prof, const DecStreams *ds) {
  DecWs ws = ws_in;
  ws.lane_q = nullptr;   // (plain per-lane records, as in launch_region)
  StreamWinWords sw;
  sw.stream_of = d_words.stream_of; sw.org = d_words.org; sw.row_end = d_words.row_end; sw.list = d_words.list;
  sw.index_rows = d_words.index_rows;
  sw.walk_rows = d_words.scratch; sw.walk_st = sw.walk_rows + n_streams; sw.wstat = sw.walk_st + n_streams;
  const WindowExtents e = window_extents(g, n_windows, h_org, 8, w, h);
  launch_zero(g, ws, n_streams, stream, prof);
  hipStream_t ws_ = side_fork(ds, stream);
  prof_begin(prof, d_row_index ? "k_stream_set_index" : "k_stream_rowwalk", ws_);
  if (d_row_index)
    hipLaunchKernelGGL(k_stream_set_index, dim3(n_streams), dim3(256), 0, ws_, g, ws, d_row_index, d_sizes, sw);
  else
    hipLaunchKernelGGL(k_stream_rowwalk, dim3(n_streams), dim3(64), 0, ws_, g, ws, d_packed, in_stride, d_sizes, sw);
  prof_end(prof, ws_);
  side_walked(ds);
  HIMG_LAUNCH(k_dec_parse, dim3(n_streams), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes);
  launch_lres_chain(g, ws, n_streams, d_packed, in_stride, d_sizes, stream, prof);
  side_join(ds, stream);
  HIMG_LAUNCH(k_stream_gate, dim3((n_windows + 63) / 64), dim3(64), g, ws, sw, h, n_windows);
  const CountRule cr = count_rule(g, list_rows, true);
  if (cr.wave) {
    HIMG_LAUNCH(k_stream_count_w, dim3(n_list), dim3(kDecThreads), cr.g, ws, d_packed, in_stride, d_sizes, sw);
  } else {
    HIMG_LAUNCH(k_stream_count, dim3(n_list), dim3(kDecThreads), cr.g, ws, d_packed, in_stride, d_sizes, sw, cr.rpc);
  }
  const int smax = region_strip_tiles(g);
  const int nstrip = (e.ntiles + smax - 1) / smax, swt = (e.ntiles + nstrip - 1) / nstrip;
  RegionArgs ra;
  ra.org = sw.org; ra.sw = swt; ra.w = w; ra.h = h; ra.out = d_out;
  prof_begin(prof, "k_dec_stream_region", stream);
  hipLaunchKernelGGL(k_dec_stream_region, dim3(nstrip, e.nrows, n_windows), dim3(kDecThreads), region_layout(g.C, swt).total,
                     stream, g, ws, d_packed, in_stride, d_sizes, ra, sw.stream_of, sw.wstat);
  prof_end(prof, stream);
  HIMG_LAUNCH(k_stream_status, dim3((n_windows + 63) / 64), dim3(64), ws, sw, d_status, n_windows);
}

// Opened streams (the kernels' comment above).  ws: the handle's products and records, with the context's LRES
// scratch (lres_sym, spec_*) beside them.  The head as launch_stream_regions runs it, the walk to the end of
// every stream's chunk beside it.
void launch_open_streams(const Geom &g, const DecWs &ws_in, int n_streams, const uint8_t *d_packed, size_t in_stride,
                         const uint32_t *d_sizes, const uint32_t *d_row_index, const OpenedWalk &walk,
                         int32_t *d_head_status, hipStream_t stream, Profiler *prof, const DecStreams *ds) {
  DecWs ws = ws_in;
  ws.lane_q = nullptr;
  launch_zero(g, ws, n_streams, stream, prof);
  hipStream_t ws_ = side_fork(ds, stream);
  prof_begin(prof, d_row_index ? "k_open_set_index" : "k_open_rowwalk", ws_);
  if (d_row_index)
    hipLaunchKernelGGL(k_open_set_index, dim3(n_streams), dim3(256), 0, ws_, g, ws, d_row_index, d_sizes, walk.rows, walk.st);
  else
    hipLaunchKernelGGL(k_open_rowwalk, dim3(n_streams), dim3(64), 0, ws_, g, ws, d_packed, in_stride, d_sizes, walk.rows,
                       walk.st);
  prof_end(prof, ws_);
  side_walked(ds);
  HIMG_LAUNCH(k_dec_parse, dim3(n_streams), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes);
  launch_lres_chain(g, ws, n_streams, d_packed, in_stride, d_sizes, stream, prof);
  side_join(ds, stream);
  const size_t n_rec = (size_t)n_streams * g.rows;
  HIMG_LAUNCH(k_open_finish, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), g, ws, d_head_status, n_streams);
}

// A call on the handle: the gate, the counts over the list (n_list = 0: none), the row kernel.  ws: the handle's.
// The gate over rectangles of height hf at the full-resolution origins d_org, then the counts.  ws: lane_q cleared.
static void launch_opened_gate_counts(const Geom &g, const DecWs &ws, const uint8_t *d_packed, size_t in_stride,
                                      const uint32_t *d_sizes, const OpenedWalk &walk, const int32_t *d_stream_of,
                                      const int32_t *d_org, const int32_t *d_list, int n_windows, int n_list,
                                      long long list_rows, int hf, int32_t *d_status, hipStream_t stream, Profiler *prof) {
  HIMG_LAUNCH(k_opened_gate, dim3((n_windows + 63) / 64), dim3(64), g, ws, d_stream_of, d_org, walk.rows, walk.st, d_status,
              hf, n_windows);
  if (n_list > 0) {
    StreamWinWords sw = {};
    sw.stream_of = d_stream_of; sw.org = d_org; sw.list = d_list;
    sw.walk_rows = walk.rows; sw.walk_st = walk.st;
    const CountRule cr = count_rule(g, list_rows, true);
    if (cr.wave) {
      HIMG_LAUNCH(k_stream_count_w, dim3(n_list), dim3(kDecThreads), cr.g, ws, d_packed, in_stride, d_sizes, sw);
    } else {
      HIMG_LAUNCH(k_stream_count, dim3(n_list), dim3(kDecThreads), cr.g, ws, d_packed, in_stride, d_sizes, sw, cr.rpc);
    }
  }
}

void launch_opened_regions(const Geom &g, const DecWs &ws_in, const uint8_t *d_packed, size_t in_stride,
                           const uint32_t *d_sizes, const OpenedWalk &walk, const int32_t *d_stream_of,
                           const int32_t *d_org, const int32_t *d_list, int n_windows, const int32_t *h_org, int n_list,
                           long long list_rows, int w, int h, uint8_t *d_out, int32_t *d_status, hipStream_t stream,
                           Profiler *prof) {
  DecWs ws = ws_in;
  ws.lane_q = nullptr;
  const WindowExtents e = window_extents(g, n_windows, h_org, 8, w, h);
  launch_opened_gate_counts(g, ws, d_packed, in_stride, d_sizes, walk, d_stream_of, d_org, d_list, n_windows, n_list,
                            list_rows, h, d_status, stream, prof);
  const int smax = region_strip_tiles(g);
  const int nstrip = (e.ntiles + smax - 1) / smax, swt = (e.ntiles + nstrip - 1) / nstrip;
  RegionArgs ra;
  ra.org = d_org; ra.sw = swt; ra.w = w; ra.h = h; ra.out = d_out;
  prof_begin(prof, "k_dec_stream_region", stream);
  hipLaunchKernelGGL(k_dec_stream_region, dim3(nstrip, e.nrows, n_windows), dim3(kDecThreads), region_layout(g.C, swt).total,
                     stream, g, ws, d_packed, in_stride, d_sizes, ra, d_stream_of, d_status);
  prof_end(prof, stream);
}

// A scaled call on the handle.  scale_log2 = 1, 2: h_org / d_org are the origins of the full-resolution rectangles
// the windows cover, (F x_k, F y_k), as in launch_region; the gate and the counts take them with the height F h,
// then the scaled row kernel runs over (strip, row, window).  scale_log2 = 3: d_org holds the origins in the
// 1/8-scale picture, and k_opened_preview_region runs alone (d_list, h_org unused).
void launch_opened_scaled_regions(const Geom &g, const DecWs &ws_in, const uint8_t *d_packed, size_t in_stride,
                                  const uint32_t *d_sizes, const OpenedWalk &walk, int scale_log2,
                                  const int32_t *d_stream_of, const int32_t *d_org, const int32_t *d_list, int n_windows,
                                  const int32_t *h_org, int n_list, long long list_rows, int w, int h, uint8_t *d_out,
                                  int32_t *d_status, hipStream_t stream, Profiler *prof) {
  DecWs ws = ws_in;
  ws.lane_q = nullptr;
  if (scale_log2 == 3) {
    PreviewWinArgs pa;
    pa.stream_of = d_stream_of; pa.org = d_org; pa.w = w; pa.h = h; pa.out = d_out; pa.status = d_status;
    const uint32_t n = (uint32_t)w * (uint32_t)h;
    HIMG_LAUNCH(k_opened_preview_region, dim3((n + 255u) / 256u, n_windows), dim3(256), g, ws, pa);
    return;
  }
  const int F = 1 << scale_log2;
  const WindowExtents e = window_extents(g, n_windows, h_org, 8 / F, w, h);
  launch_opened_gate_counts(g, ws, d_packed, in_stride, d_sizes, walk, d_stream_of, d_org, d_list, n_windows, n_list,
                            list_rows, F * h, d_status, stream, prof);
  const int smax = scaled_strip_tiles(g, scale_log2);
  const int nstrip = (e.ntiles + smax - 1) / smax, swt = (e.ntiles + nstrip - 1) / nstrip;
  ScaledRegionArgs sa;
  sa.org = d_org; sa.sw = swt; sa.w = w; sa.h = h; sa.out = d_out;
  const dim3 grid(nstrip, e.nrows, n_windows);
  prof_begin(prof, "k_dec_opened_scaled_region", stream);
  if (scale_log2 == 1)
    hipLaunchKernelGGL(k_dec_opened_scaled_region<4>, grid, dim3(kDecThreads), scaled_layout<4>(g.C, swt).total, stream, g,
                       ws, d_packed, in_stride, d_sizes, sa, d_stream_of, d_status);
  else
    hipLaunchKernelGGL(k_dec_opened_scaled_region<2>, grid, dim3(kDecThreads), scaled_layout<2>(g.C, swt).total, stream, g,
                       ws, d_packed, in_stride, d_sizes, sa, d_stream_of, d_status);
  prof_end(prof, stream);
}

// What the row-span decodes share behind their gates and walks: the fill over w.kfill, the counts and the row
// kernel over rows [w.k0, w.k1), every load bounded by w.bound.  cmap: the concealing decode's row map, or
// nullptr.  k1 is known on the device alone, so the grids cover all rows and a workgroup outside its frame's
// span returns at once.
static void launch_span_rows(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                             const SpanWords &w, uint8_t *d_cmap, uint8_t *d_out, hipStream_t stream, Profiler *prof) {
  // The rows that have not arrived: the low-res plane and kfill are all the fill needs.
  HIMG_LAUNCH(k_prefix_fill, dim3((2 * g.cols + 255) / 256, g.rows, batch), dim3(256), g, ws, w.kfill, d_out);
  // Every complete row gets a record (launch_region's rule).
  const CountRule cr = count_rule(g, (long long)batch * g.rows, true);
  if (cr.wave) {
    HIMG_LAUNCH(k_span_count_w, dim3((g.rows + kCountRowsW - 1) / kCountRowsW, batch), dim3(kDecThreads), cr.g, ws,
                d_packed, in_stride, w.bound, w.k0, w.k1);
  } else {
    HIMG_LAUNCH(k_span_count, dim3((g.rows + cr.rpc - 1) / cr.rpc, batch), dim3(kDecThreads), cr.g, ws, d_packed,
                in_stride, w.bound, w.k0, w.k1, cr.rpc);
  }
  const int smax = region_strip_tiles(g);
  const int nstrip = (g.cols + smax - 1) / smax, sw = (g.cols + nstrip - 1) / nstrip;
  SpanArgs sa;
  sa.k0 = w.k0; sa.k1 = w.k1; sa.cmap = d_cmap; sa.sw = sw; sa.out = d_out;
  const dim3 grid(nstrip, g.rows, batch);
  const uint32_t lds = region_layout(g.C, sw).total;
  prof_begin(prof, d_cmap ? "k_dec_span<true>" : "k_dec_span<false>", stream);
  if (d_cmap)
    hipLaunchKernelGGL(k_dec_span<true>, grid, dim3(kDecThreads), lds, stream, g, ws, d_packed, in_stride, w.bound, sa);
  else
    hipLaunchKernelGGL(k_dec_span<false>, grid, dim3(kDecThreads), lds, stream, g, ws, d_packed, in_stride, w.bound, sa);
  prof_end(prof, stream);
}

// The decode of stream prefixes, fresh (d_state == nullptr) or continued from the states.  d_words: 8 x batch
// words -- the bytes present (staged by the caller), then what k_span_gate and k_span_rowwalk leave for the
// kernels behind them (SpanWords).
void launch_prefix(const Geom &g, const DecWs &ws_in, int batch, const uint8_t *d_packed, size_t in_stride,
                   uint32_t *d_words, PfxState *d_state, uint8_t *d_out, int32_t *d_rows, int32_t *d_status,
                   hipStream_t stream, Profiler *prof, const DecStreams *ds) {
  DecWs ws = ws_in;
  ws.lane_q = nullptr;   // (plain per-lane records, as in launch_region)
  const size_t n = (size_t)batch;
  SpanWords w;
  w.avail = d_words; w.tx = d_words + n; w.bound = d_words + 2 * n;
  w.k0 = (int32_t *)(d_words + 3 * n); w.k1 = (int32_t *)(d_words + 4 * n);
  w.gate = (int32_t *)(d_words + 5 * n); w.kfill = (int32_t *)(d_words + 6 * n);
  w.pos = d_words + 7 * n;
  const dim3 per_frame((batch + 63) / 64), b64(64);
  launch_zero(g, ws, batch, stream, prof);
  HIMG_LAUNCH(k_span_gate, dim3(batch), b64, g, ws, d_packed, in_stride, d_state, w);
  // The row headers on the side stream beside k_dec_parse_prefix and the LRES chain (launch_region's fork).
  hipStream_t ws_ = side_fork(ds, stream);
  prof_begin(prof, "k_span_rowwalk", ws_);
  hipLaunchKernelGGL(k_span_rowwalk, per_frame, b64, 0, ws_, g, ws, d_packed, in_stride, w, batch);
  prof_end(prof, ws_);
  side_walked(ds);
  HIMG_LAUNCH(k_dec_parse_prefix, dim3(batch), dim3(kParseThreads), g, ws, d_packed, in_stride, w.tx, w.bound);
  launch_lres_chain(g, ws, batch, d_packed, in_stride, w.bound, stream, prof);
  side_join(ds, stream);
  launch_span_rows(g, ws, batch, d_packed, in_stride, w, nullptr, d_out, stream, prof);
  HIMG_LAUNCH(k_span_status, per_frame, b64, ws, w, d_state, d_status, d_rows, batch);
}

// The concealing decode.  d_words: 5 x batch words -- the packed sizes (staged by the caller), then the full
// decode's status words, k_f, the gate's classes and the zeros that are the span's k0; d_cmap: batch x rows
// bytes.  Pass one is launch_decode as himg_hip_decode_device calls it; pass two runs behind it on the
// caller's stream.
void launch_conceal(const Geom &g, const DecWs &ws_in, int batch, const uint8_t *d_packed, size_t in_stride,
                    uint32_t *d_words, uint8_t *d_cmap, uint8_t *d_out, int32_t *d_concealed, uint8_t *d_rowmap,
                    int32_t *d_status, hipStream_t stream, Profiler *prof, const HostOpts &ho, const DecStreams *ds) {
  const size_t n = (size_t)batch;
  const uint32_t *d_sizes = d_words;
  int32_t *d_st1 = (int32_t *)(d_words + n), *d_k = (int32_t *)(d_words + 2 * n);
  int32_t *d_act = (int32_t *)(d_words + 3 * n);
  SpanWords w = {};   // (no gate of the prefix decode's: the loads are bounded by the packed sizes)
  w.bound = d_words; w.k0 = (int32_t *)(d_words + 4 * n); w.k1 = d_k; w.kfill = d_k;
  launch_decode(g, ws_in, batch, d_packed, in_stride, d_sizes, d_out, d_st1, stream, prof, ho, ds, 0, g.rows);
  DecWs ws = ws_in;
  ws.lane_q = nullptr;   // (plain per-lane records, as in launch_region: they overwrite the full decode's)
  const dim3 per_frame((batch + 63) / 64), b64(64);
  HIMG_LAUNCH(k_conceal_gate, per_frame, b64, ws, d_st1, w.k0, d_k, d_act, batch);
  const uint32_t n16 = (uint32_t)(ws.lres_stride / 16);
  HIMG_LAUNCH(k_conceal_zero, dim3(n16 / 256 < 64 ? (n16 + 255) / 256 : 64, batch), dim3(256), ws, d_act);
  launch_lres_chain(g, ws, batch, d_packed, in_stride, d_sizes, stream, prof);
  HIMG_LAUNCH(k_conceal_rowwalk, per_frame, b64, g, ws, d_packed, in_stride, d_act, d_k, batch);
  HIMG_LAUNCH(k_conceal_map, dim3((unsigned)(((size_t)batch * g.rows + 255) / 256)), dim3(256), d_act, d_k, d_cmap, g.rows,
              batch);
  launch_span_rows(g, ws, batch, d_packed, in_stride, w, d_cmap, d_out, stream, prof);
  HIMG_LAUNCH(k_conceal_status, dim3(batch), b64, ws, d_st1, d_act, d_cmap, g.rows, d_rowmap, d_status, d_concealed);
}

void launch_scaled(const Geom &g, const DecWs &ws_in, int batch, const uint8_t *d_packed, size_t in_stride,
                   const uint32_t *d_sizes, const uint32_t *d_row_index, int scale_log2, uint8_t *d_out,
                   int32_t *d_status, hipStream_t stream, Profiler *prof, const DecStreams *ds) {
  constexpr int kWalkAll = 0x7fffffff;
  DecWs ws = ws_in;
  ws.lane_q = nullptr;   // (plain per-lane records: no quarter records for k_row_count<false>)
  const int F = 1 << scale_log2;
  launch_zero(g, ws, batch, stream, prof);
  // launch_decode's order: the whole row index on the side stream beside k_dec_parse, the counts
  // behind both on the side stream beside the LRES chain, the row kernel behind the join.
  hipStream_t side = ds ? ds->side : stream;
  auto walk = [&](hipStream_t s) {
    prof_begin(prof, d_row_index ? "k_dec_set_index" : "k_dec_rowwalk", s);
    if (d_row_index)   // (one frame: himg_hip_decode_scaled_to)
      hipLaunchKernelGGL(k_dec_set_index, dim3(1), dim3(256), 0, s, g, ws, d_row_index, d_sizes, 0, g.rows);
    else
      hipLaunchKernelGGL(k_dec_rowwalk, dim3(batch), dim3(64), 0, s, g, ws, d_packed, in_stride, d_sizes, kWalkAll, 0);
    prof_end(prof, s);
  };
  // Every row gets one record: the count kernels that read the payload in place (launch_region's reasons).
  const CountRule cr = count_rule(g, (long long)batch * g.rows, true);
  auto row_count = [&](hipStream_t s) {
    prof_begin(prof, "k_row_count", s);
    if (cr.wave)
      launch_row_count_w(cr.g, ws, batch, d_packed, in_stride, d_sizes, 0, g.rows, s);
    else
      hipLaunchKernelGGL(k_row_count<false>, dim3((g.rows + cr.rpc - 1) / cr.rpc, batch), dim3(kDecThreads), 0, s, cr.g, ws,
                         d_packed, in_stride, d_sizes, 0, g.rows, cr.rpc);
    prof_end(prof, s);
  };
  if (ds) {
    (void)hipEventRecord(ds->ev_fork, stream);
    (void)hipStreamWaitEvent(side, ds->ev_fork, 0);
    walk(side);
  }
  HIMG_LAUNCH(k_dec_parse, dim3(batch), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes);
  if (ds) {
    (void)hipEventRecord(ds->ev_fork, stream);
    (void)hipStreamWaitEvent(side, ds->ev_fork, 0);
    row_count(side);
    (void)hipEventRecord(ds->ev_cnt[0], side);
  } else {
    walk(stream);
  }
  launch_lres_chain(g, ws, batch, d_packed, in_stride, d_sizes, stream, prof);
  if (ds) (void)hipStreamWaitEvent(stream, ds->ev_cnt[0], 0);
  else row_count(stream);
  ScaledArgs sa;
  const uint32_t lds_one = scale_log2 == 1 ? scaled_layout_one<4>(g.C, g.cols).total : scaled_layout_one<2>(g.C, g.cols).total;
  const bool one = lds_one <= kLdsMax - 1024u;   // (room for the kernel's static LDS)
  const int smax = scaled_strip_tiles(g, scale_log2), nstrip = one ? 1 : (g.cols + smax - 1) / smax;
  sa.sw = (g.cols + nstrip - 1) / nstrip;   // (strips of equal width)
  sa.ow = (g.W + F - 1) / F; sa.oh = (g.H + F - 1) / F; sa.out = d_out;
  prof_begin(prof, "k_dec_scaled", stream);
#define HIMG_SCALED_LAUNCH(S_, ONE_, LDS_)                                                                        \
  hipLaunchKernelGGL((k_dec_scaled<S_, ONE_>), dim3(nstrip, g.rows, batch), dim3(kDecThreads), LDS_, stream, g, ws, \
                     d_packed, in_stride, d_sizes, sa)
  if (scale_log2 == 1 && one) HIMG_SCALED_LAUNCH(4, true, lds_one);
  else if (scale_log2 == 1) HIMG_SCALED_LAUNCH(4, false, scaled_layout<4>(g.C, sa.sw).total);
  else if (one) HIMG_SCALED_LAUNCH(2, true, lds_one);
  else HIMG_SCALED_LAUNCH(2, false, scaled_layout<2>(g.C, sa.sw).total);
#undef HIMG_SCALED_LAUNCH
  prof_end(prof, stream);
  HIMG_LAUNCH(k_dec_status, dim3((batch + 63) / 64), dim3(64), ws, d_status, batch);
}

void launch_row_records(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                        const uint32_t *d_sizes, int32_t *d_status, hipStream_t stream, Profiler *prof) {
  launch_zero(g, ws, batch, stream, prof);
  HIMG_LAUNCH(k_dec_parse, dim3(batch), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes);
  HIMG_LAUNCH(k_dec_rowwalk, dim3(batch), dim3(64), g, ws, d_packed, in_stride, d_sizes, 0x7fffffff, 0);
  prof_begin(prof, "k_row_count", stream);
  launch_row_count_w(g, ws, batch, d_packed, in_stride, d_sizes, 0, g.rows, stream);
  prof_end(prof, stream);
  HIMG_LAUNCH(k_dec_status, dim3((batch + 63) / 64), dim3(64), ws, d_status, batch);
}

// The stage name of a store kernel of launch_decode.  The forms with a descriptor carry their
// instantiation in the name: the tests assert which one ran.
enum StoreInst { kRow512, kRowWhole4, kRowAny, kTileFast, kTileAny };
static const char *store_stage_name(StoreKind kind, StoreInst inst) {
  static const char *const kName[5][5] = {
      {"k_dec_row_fused", "k_dec_row_fused", "k_dec_row_fused", "k_tile_inv<true>", "k_tile_inv<false>"},
      {"k_dec_row_fused_t<512>", "k_dec_row_fused_t<-1>", "k_dec_row_fused_t<0>", "k_tile_inv_t<true>", "k_tile_inv_t<false>"},
      {"k_dec_row_fused_p<512>", "k_dec_row_fused_p<-1>", "k_dec_row_fused_p<0>", "k_tile_inv_p<true>", "k_tile_inv_p<false>"},
      {"k_dec_row_fused_m<512>", "k_dec_row_fused_m<-1>", "k_dec_row_fused_m<0>", "k_tile_inv_m<true>", "k_tile_inv_m<false>"},
      {"k_dec_row_fused_c<512>", "k_dec_row_fused_c<-1>", "k_dec_row_fused_c<0>", "k_tile_inv_c<true>", "k_tile_inv_c<false>"}};
  return kName[kind][inst];
}

// The fused row kernel in the requested form over n_wg workgroups.  The forms with a descriptor have
// <512>, <-1> -- which also serves 2048 and 1920 -- and <0>.
template <int COLS>
static void launch_row_fused(const StoreForm &form, const RowArgs &ra, unsigned n_wg, uint32_t lds, hipStream_t stream,
                             Profiler *prof) {
  constexpr int FC = COLS == 256 || COLS == 240 ? -1 : COLS;
  const dim3 grid(n_wg), block(kDecThreads);
  prof_begin(prof, store_stage_name(form.kind, FC == 512 ? kRow512 : FC == -1 ? kRowWhole4 : kRowAny), stream);
  if (form.kind == kStoreTens) {
    const RowArgsT rt = {ra, form.tens()};
    hipLaunchKernelGGL((k_dec_row_fused_t<FC>), grid, block, lds, stream, rt);
  } else if (form.kind == kStorePitch) {
    const RowArgsP rp = {ra, form.dst()};
    hipLaunchKernelGGL((k_dec_row_fused_p<FC>), grid, block, lds, stream, rp);
  } else if (form.kind == kStorePyr) {
    const RowArgsM rm = {ra, form.pyr()};
    hipLaunchKernelGGL((k_dec_row_fused_m<FC>), grid, block, lds, stream, rm);
  } else if (form.kind == kStorePlanes) {
    const RowArgsC rc = {ra, form.planes()};
    hipLaunchKernelGGL((k_dec_row_fused_c<FC>), grid, block, lds, stream, rc);
  } else {
    hipLaunchKernelGGL((k_dec_row_fused<COLS>), grid, block, lds, stream, ra);
  }
  prof_end(prof, stream);
}

// k_tile_inv in the requested form over block rows v0, v0 + 1, ... (grid.y of them).
template <bool FAST>
static void launch_tile_inv(const StoreForm &form, const Geom &g, const DecWs &ws, uint8_t *d_out, int v0, dim3 grid,
                            hipStream_t stream, Profiler *prof) {
  const dim3 block(256);
  prof_begin(prof, store_stage_name(form.kind, FAST ? kTileFast : kTileAny), stream);
  if (form.kind == kStoreTens) {
    const TileArgsT ta = {g, ws, d_out, v0, form.tens()};
    hipLaunchKernelGGL(k_tile_inv_t<FAST>, grid, block, 0, stream, ta);
  } else if (form.kind == kStorePitch) {
    const TileArgsP tp = {g, ws, d_out, v0, form.dst()};
    hipLaunchKernelGGL(k_tile_inv_p<FAST>, grid, block, 0, stream, tp);
  } else if (form.kind == kStorePyr) {
    const TileArgsM tm = {g, ws, v0, form.pyr()};
    hipLaunchKernelGGL(k_tile_inv_m<FAST>, grid, block, 0, stream, tm);
  } else if (form.kind == kStorePlanes) {
    const TileArgsC tc = {g, ws, d_out, v0, form.planes()};
    hipLaunchKernelGGL(k_tile_inv_c<FAST>, grid, block, 0, stream, tc);
  } else {
    hipLaunchKernelGGL(k_tile_inv<FAST>, grid, block, 0, stream, g, ws, d_out, v0);
  }
  prof_end(prof, stream);
}

void launch_decode(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed,
                   size_t in_stride, const uint32_t *d_sizes, uint8_t *d_out,
                   int32_t *d_status, hipStream_t stream, Profiler *prof, const HostOpts &ho,
                   const DecStreams *ds, int r0, int r1,
                   const uint32_t *d_row_index, bool index_only, int phase, const StoreForm &form) {
  // d_row_index: the FRES row index is given (k_dec_set_index instead of the serial
  // header walk; one frame).  index_only: container parse and row-header walk only --
  // the caller reads ws.row_off / ws.row_len / DecFrame::rows_first (rank 0 of a
  // row-sharded decode); with r1 == 0 the walk stops in front of the first row header
  // (rows_first alone: what a rank needs to send the head of the stream on its way).
  // phase: kDecHead = what needs only the head of the stream (container parse, LRES chain,
  // predictor inverse), kDecRows = the FRES rows (index, counts, row kernels, verdict);
  // a row-sharded decode launches them one by one, the rows once their bytes have arrived.
  constexpr int kWalkAll = 0x7fffffff;
  const bool do_head = (phase & kDecHead) != 0, do_rows = (phase & kDecRows) != 0;
  if (index_only) {
    HIMG_LAUNCH(k_dec_parse, dim3(batch), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes);
    HIMG_LAUNCH(k_dec_rowwalk, dim3(batch), dim3(64), g, ws, d_packed, in_stride, d_sizes, r1 == 0 ? 0 : kWalkAll, 0);
    HIMG_LAUNCH(k_dec_status, dim3((batch + 63) / 64), dim3(64), ws, d_status, batch);
    return;
  }
  // Block rows [r0, r1) only (row-sharded decode: every rank decodes the small
  // LRES stream and walks all row headers, then its own FRES rows).
  const int nrows = r1 - r0;
  const CountRule cr = count_rule(g, (long long)batch * nrows, false);
  const unsigned gx = (unsigned)((((g.cols + 31) / 32) * 64 + 255) / 256);   // k_tile_inv: two lanes per tile, 32 tiles per wave
  // Fused row kernel when the row's symbols and the decode tables fit the 160 KiB
  // LDS (width <= 4352 for RGBA); the payload is read in place from L2.
  const int wps = (ho.allow_fused && fused_layout(g.row_block).total <= kLdsMax) ? 1 : 0;
  // A single large frame (nothing else to fill the GPU with while one lane walks its row
  // headers, 1.3 ms for 16384 x 16384): the rows in two ranges -- the walk of a range on
  // `side`, its counts on `side2`, its row kernels on the caller's stream, each behind the
  // stage before it and beside the next range's walk.  16384^2: 4.15 -> 3.32 ms, which is
  // the sum of the row kernels' own times (two ranges or four); a dependency across
  // streams costs tens of microseconds, so frames of fewer than 1024 block rows (4096^2:
  // 0.40 ms either way, 1024^2: 0.23 -> 0.30 ms) stay in one piece.
  const int seg_env = ho.walk_segs;
  const int seg_want = seg_env ? (seg_env < 1 ? 1 : seg_env > kWalkSegs ? kWalkSegs : seg_env)
                               : (nrows >= 1024 ? (wps ? 2 : kWalkSegs) : 1);   // (rows through windows: three kernels per range in a pipeline)
  const int nseg = (ds && batch == 1 && !d_row_index && r0 == 0 && r1 == g.rows && nrows >= 16 * kWalkSegs) ? seg_want : 1;
  hipStream_t side = ds ? ds->side : nullptr;
  hipStream_t cnt_stream = !ds ? stream : nseg > 1 ? ds->side2 : ds->side;
  auto seg_lo = [&](int k) { return r0 + (int)((long long)nrows * k / nseg); };
  // Diagnostics and the LRES symbols (k_lres_write stores the non-zero ones only) are
  // cleared up front: k_row_count may start as soon as the parse and the walk are done.
  if (do_head) launch_zero(g, ws, batch, stream, prof);
  // Fork: the serial FRES row-header walk runs on the side stream beside k_dec_parse.
  if (ds && do_rows) {
    (void)hipEventRecord(ds->ev_fork, stream);
    (void)hipStreamWaitEvent(side, ds->ev_fork, 0);
    if (d_row_index) {
      prof_begin(prof, "k_dec_set_index", side);
      hipLaunchKernelGGL(k_dec_set_index, dim3(1), dim3(256), 0, side, g, ws, d_row_index, d_sizes, r0, r1);
      prof_end(prof, side);
      (void)hipEventRecord(ds->ev_walk[0], side);
    } else {
      for (int k = 0; k < nseg; ++k) {
        prof_begin(prof, "k_dec_rowwalk", side);
        hipLaunchKernelGGL(k_dec_rowwalk, dim3(batch), dim3(64), 0, side, g, ws, d_packed, in_stride, d_sizes,
                           k + 1 < nseg ? seg_lo(k + 1) : kWalkAll, k > 0 ? 1 : 0);
        prof_end(prof, side);
        (void)hipEventRecord(ds->ev_walk[k], side);
      }
    }
  }
  if (do_head) HIMG_LAUNCH(k_dec_parse, dim3(batch), dim3(kParseThreads), g, ws, d_packed, in_stride, d_sizes);
  // The FRES counts need the decode tables (parse) and the row index (walk); their
  // stream joins this one again before the FRES row kernels.
  // (ds == nullptr: everything in line.)
  // (Which count kernel: count_rule.)
  auto row_count = [&](hipStream_t s, int a, int b) {
    if (b <= a) return;
    prof_begin(prof, "k_row_count", s);
    if (cr.wave)
      launch_row_count_w(g, ws, batch, d_packed, in_stride, d_sizes, a, b, s);
    else if (wps)
      hipLaunchKernelGGL(k_row_count<true>, dim3((b - a + cr.rpc - 1) / cr.rpc, batch), dim3(kDecThreads), 0, s, g, ws,
                         d_packed, in_stride, d_sizes, a, b, cr.rpc);
    else if (ws.lane_q && g.wide_q && g.count_wave < 0 && (g.row_block % 16) == 0)
      // Rows that go through windows, at a bit rate the staged reader takes (the host's estimate
      // from the stream's size; a row beyond it is left to k_dec_huff): four records per lane
      // from 4096 sub-sequences.  HIMG_OPT_COUNT_WAVE = 0 / 1 force the other two forms.
      hipLaunchKernelGGL(k_row_count_q, dim3(b - a, batch), dim3(kDecThreads), 0, s, g, ws, d_packed, in_stride, d_sizes, a);
    else
      hipLaunchKernelGGL(k_row_count<false>, dim3((b - a + cr.rpc - 1) / cr.rpc, batch), dim3(kDecThreads), 0, s, g, ws,
                         d_packed, in_stride, d_sizes, a, b, cr.rpc);
    prof_end(prof, s);
  };
  // The entropy pass of rows that do not fit the LDS, rows [a, b): every 128 KiB window of a
  // row's symbols is assembled in LDS (k_row_window) and stored whole; rows whose block is not a
  // multiple of 16 bytes (ragged widths of 1-3 channel frames) and rows without a usable
  // record take k_dec_huff's 32 KiB windows (which skips the others).
  const bool window = (g.row_block % 16) == 0;
  auto window_pass = [&](hipStream_t s, int a, int b) {
    if (b <= a) return;
    if (window) {
      const unsigned nwin = (unsigned)(((uint32_t)g.row_block + kRowWindow - 1u) / kRowWindow);
      prof_begin(prof, "k_row_window", s);
      hipLaunchKernelGGL(k_row_window, dim3(nwin, b - a, batch), dim3(kDecThreads), kRowWindowLds, s, g, ws, d_packed,
                         in_stride, d_sizes, a);
      prof_end(prof, s);
    }
    prof_begin(prof, "k_dec_huff", s);
    hipLaunchKernelGGL(k_dec_huff, dim3(b - a, batch), dim3(kDecThreads), 0, s, g, ws, d_packed, in_stride,
                       d_sizes, 1 + a, 1, window ? 2 : 1);
    prof_end(prof, s);
  };
  if (!do_rows) {
    // (nothing of the rows in this launch)
  } else if (ds) {
    (void)hipEventRecord(ds->ev_fork, stream);
    (void)hipStreamWaitEvent(cnt_stream, ds->ev_fork, 0);
    // They fill the CUs the latency-bound LRES kernels leave idle.
    for (int k = 0; k < nseg; ++k) {
      if (cnt_stream != side) (void)hipStreamWaitEvent(cnt_stream, ds->ev_walk[k], 0);
      row_count(cnt_stream, seg_lo(k), seg_lo(k + 1));
      // Rows that go through HBM: their entropy pass (k_row_window, k_dec_huff) needs the
      // stream's tables and the counts, NOT the low-res plane -- it follows the counts on
      // their stream, beside the LRES chain on the caller's, and only the transform waits for
      // both.  (Behind the LRES chain on the caller's stream these kernels were the critical
      // path of a single large frame: LRES chain 1.1 ms, then 1.8 ms of window / transform
      // launches one after the other -- 16384^2: 2.88 -> see DESIGN.md.)
      (void)hipEventRecord(ds->ev_cnt[k], cnt_stream);
      if (!wps) {
        // ... on a stream of its own where there are several row ranges: the counts of the next
        // range start when its walk is done, not behind this range's windows.
        hipStream_t ws_ = (nseg > 1 && ds->side3) ? ds->side3 : cnt_stream;
        if (ws_ != cnt_stream) (void)hipStreamWaitEvent(ws_, ds->ev_cnt[k], 0);
        window_pass(ws_, seg_lo(k), seg_lo(k + 1));
        (void)hipEventRecord(ds->ev_win[k], ws_);
      }
    }
  } else if (d_row_index) {
    HIMG_LAUNCH(k_dec_set_index, dim3(1), dim3(256), g, ws, d_row_index, d_sizes, r0, r1);
  } else {
    HIMG_LAUNCH(k_dec_rowwalk, dim3(batch), dim3(64), g, ws, d_packed, in_stride, d_sizes, kWalkAll, 0);
  }
  if (do_head) launch_lres_chain(g, ws, batch, d_packed, in_stride, d_sizes, stream, prof);
  // The pyramid's 1/8-scale level: the low-res plane the chain has just finished, as launch_preview
  // stores it.  (A frame the rows reject later keeps these bytes: a failed frame's are unspecified.)
  if (do_head && form.kind == kStorePyr && form.pyr().level[3]) {
    const uint32_t npix = (uint32_t)g.rows * (uint32_t)g.cols;
    HIMG_LAUNCH(k_lres_preview, dim3((npix + 1023u) / 1024u, batch), dim3(256), g, ws, form.pyr().level[3]);
  }
  const bool whole4 = g.C == 4 && (g.W & 7) == 0 && (g.H & 7) == 0;   // FULL4 / FAST
  if (!do_rows) return;
  if (wps) {
    // Rows per workgroup: as many as the transform has lanes for and the LDS holds
    // (4096-pixel rows: one).
    const int per_row = ((g.cols + 31) / 32) * 64;
    int rpw = 1;
    while (rpw < 8 && (rpw + 1) * per_row <= kDecThreads && fused_layout(g.row_block, rpw + 1).total <= kLdsMax) ++rpw;
    if (g.W == 4096 && g.C == 4 && (g.H & 7) == 0) rpw = 1;
    const uint32_t lds = fused_layout(g.row_block, rpw).total;
    // Persistent workgroups (HIMG_PERSIST_ROWS=0: one workgroup per grid element as before): as
    // many as run at once -- one per CU.
    // (Sixteen wavefronts of 120+ registers each: one workgroup per CU whatever the LDS leaves.)
    const int n_cu = ho.n_cu, per_cu = 1;
    const int slots = ho.persist_rows > 1 ? ho.persist_rows : n_cu * per_cu;
    RowArgs ra;
    ra.g = g; ra.ws = ws; ra.packed = d_packed; ra.in_stride = in_stride; ra.sizes = d_sizes;
    ra.out_frames = d_out; ra.rpw = rpw; ra.gy = batch;
    for (int k = 0; k < nseg; ++k) {
      const int a = seg_lo(k), b = seg_lo(k + 1);
      if (ds) (void)hipStreamWaitEvent(stream, ds->ev_cnt[k], 0);
      else row_count(stream, a, b);
      if (b <= a) continue;
      ra.r0 = a; ra.r1 = b; ra.gx = (b - a + rpw - 1) / rpw;
      const long long all = (long long)ra.gx * batch;
      const bool pers = ho.persist_rows != 0 && all > slots;
      ra.next_dist = pers ? 0 : n_cu * per_cu;
      const unsigned n_wg = (unsigned)(pers ? slots : all);
      if (g.W == 4096 && whole4) launch_row_fused<512>(form, ra, n_wg, lds, stream, prof);
      else if (g.W == 2048 && whole4) launch_row_fused<256>(form, ra, n_wg, lds, stream, prof);   // compile-time strides for the other
      else if (g.W == 1920 && whole4) launch_row_fused<240>(form, ra, n_wg, lds, stream, prof);   // BASELINE widths (config 3: 1920)
      else if (whole4) launch_row_fused<-1>(form, ra, n_wg, lds, stream, prof);
      else launch_row_fused<0>(form, ra, n_wg, lds, stream, prof);
    }
  } else {
    // Symbols through HBM: the entropy pass (window_pass above; with side streams it ran on the
    // counts' stream already), then the transform, which needs the low-res plane as well.
    for (int k = 0; k < nseg; ++k) {
      const int a = seg_lo(k), b = seg_lo(k + 1);
      if (ds) (void)hipStreamWaitEvent(stream, ds->ev_win[k], 0);
      else { row_count(stream, a, b); window_pass(stream, a, b); }
      if (b <= a) continue;
      if (whole4) launch_tile_inv<true>(form, g, ws, d_out, a, dim3(gx, b - a, batch), stream, prof);
      else launch_tile_inv<false>(form, g, ws, d_out, a, dim3(gx, b - a, batch), stream, prof);
    }
  }
  HIMG_LAUNCH(k_dec_status, dim3((batch + 63) / 64), dim3(64), ws, d_status, batch);
}

// ---- the encoder's distortion probe ----------------------------------------------------
void launch_sse(const Geom &g, const EncWs &ws, int batch, const uint8_t *d_frames, const QualSel &qs,
                const SseArgs &sa, hipStream_t stream, Profiler *prof) {
  const unsigned gx = (unsigned)((((g.cols + 31) / 32) * 64 + 255) / 256);   // two lanes per tile, 32 tiles per wave
  const dim3 grid(gx, g.rows, batch);
  if (g.C == 4 && g.stride == 4 && (g.W & 7) == 0 && (g.H & 7) == 0)
    HIMG_LAUNCH(k_sse<true>, grid, dim3(256), g, d_frames, ws.fres_sym, ws.fres_stride, sa.rec, ws.plane_stride, sa.tab,
                qs.quality, (unsigned long long *)sa.sse);
  else
    HIMG_LAUNCH(k_sse<false>, grid, dim3(256), g, d_frames, ws.fres_sym, ws.fres_stride, sa.rec, ws.plane_stride, sa.tab,
                qs.quality, (unsigned long long *)sa.sse);
}

// DecFrame::row_tabs on the host (k_dec_parse, identity_test_words), from the tables a stream of
// that quality carries.
void sse_fill_tab(const int16_t fmap[128], const ShiftTables &st, SseTab *t) {
  static_assert(sizeof(t->w) == kRowTabWords * 4, "DecFrame::row_tabs");
  int16_t *um = reinterpret_cast<int16_t *>(t->w);
  uint8_t *sh = reinterpret_cast<uint8_t *>(t->w + 128);
  uint32_t *sp = t->w + 160;
  for (int k = 0; k < 256; ++k) {
    const int sc = (int8_t)k;
    um[k] = (int16_t)(sc >= 0 ? fmap[sc] : (sc == -128 ? -fmap[127] : -fmap[-sc]));
  }
  for (int k = 0; k < 128; ++k) sh[k] = st.s[k >> 6][k & 63];
  for (int k = 0; k < 64; ++k) {
    const int ch = k >> 5, e = k & 31, x = e >> 2, j = e & 3;
    sp[k] = (uint32_t)st.s[ch][(2 * j) * 8 + x] | ((uint32_t)st.s[ch][(2 * j + 1) * 8 + x] << 16);
  }
  int n = 127;
  for (int i = 0; i < 128; ++i)
    if (fmap[i] != i) { n = i - 1; break; }
  for (int l = 0; l < 2; ++l) {
    int smax = 0;
    for (int y = 2; y < 8; ++y)
      for (int x = 1; x < 8; ++x) smax = st.s[l][y * 8 + x] > smax ? st.s[l][y * 8 + x] : smax;
    int B = 0;
    if (n >= 1) {
      B = 1;
      while (2 * B <= n) B *= 2;
      while (B && ((long long)B << smax) > 2048) B >>= 1;
    }
    const uint32_t b16 = B ? (uint32_t)B : 0x4000u, m16 = B ? (uint32_t)(0xffffu & ~(2u * B - 1u)) : 0xffffu;
    sp[64 + 2 * l] = b16 | (b16 << 16);
    sp[64 + 2 * l + 1] = m16 | (m16 << 16);
  }
}

}  // namespace himg_dev
