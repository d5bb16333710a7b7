// himg_dev.h -- structures shared by the HIP kernels and the host orchestration.
//
// Vocabulary (follows the reference's domain):
//   block row  : one strip of 8 pixel rows = cols tiles = row_block symbols
//   LRES / FRES: the low-res and full-res payloads before entropy coding
//   span       : a contiguous symbol range entropy-coded by one workgroup
//                (FRES: one block row; LRES: kLresSpan symbols)
#ifndef HIMG_DEV_H_
#define HIMG_DEV_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "search_step.h"

namespace himg_dev {

constexpr int kNumSym = 261;      // huffman_common.h:18-20
constexpr int kHistStride = 264;  // padded row of a histogram / code table
constexpr int kLresSpan = 16384;  // LRES symbols per entropy span
constexpr int kIterSyms = 4096;   // symbols per workgroup iteration (256 thr x 16 B)
constexpr int kTreeStride = 384;  // bytes reserved per serialised tree (max 359)
constexpr int kMaxCodeLen = 32;   // reference keeps codes in uint32_t (huffman_enc.cpp:87)
constexpr int kHeadLen = 175;     // RIFF(12)+FRMT(19)+LMAP(136)+'LRES',size(8)

struct Geom {
  int W, H, C, stride;
  int rows, cols, mrows, mcols;
  int chan_size, lres_size;  // LRES payload per channel / total
  int row_block;             // cols*C*64: FRES symbols per block row
  int ycbcr;                 // effective flag: use_ycbcr && C >= 3
  int lres_spans;            // ceil(lres_size / kLresSpan)
  int use_blocks;            // FRES: block_size < in_size (huffman_enc.cpp:256)
  int fix_t2;                // decoder, opt-in: accept the encoder's own compressible streams (see himg_hip.h)
  int lres_serial;           // decoder test knob: distrust the parallel LRES chain, take the serial fallback
  int max_sub;               // decoder: longest sub-sequence in bits (4096; tests lower it to force several chunks per stream)
  int lead_bits;             // decoder: lead-in before a lane's nominal start (lean_fixpoint; 0 = start blind)
  // Kernel variants (context options, see himg_hip.h HIMG_OPT_*): -1 = chosen by the launch size.
  int prefetch_rows;         // decoder: the row kernel touches the packed bytes of the row that takes its CU next (HIMG_PREFETCH_ROWS=0 turns it off: an A/B knob)
  int count_wave;            // decoder: k_row_count_w (a wavefront per row) instead of k_row_count
  int count_stretch;         // decoder, k_row_count_w: sub-sequences per lane (2, 4, 8; 1 = one each, the earlier form; -1 = kCountStretch)
  int wide_q;                // decoder, rows wider than the LDS: the host's estimate says a quarter sub-sequence of a row
                             // (1/4096 of its payload) fits k_row_count_q's staging buffer -- that kernel counts
  int emit_rows;             // encoder: k_emit_t<8> (a wavefront per row) instead of a workgroup per row
  int front;                 // encoder: k_front (averages + low-res plane + pixel stage in one pass over the pixels)
  int row_tokens;            // encoder: FRES rows as a token stream (k_tok -> k_emit_tok) instead of k_tok_hist / k_emit_t
                             // over the dense symbol plane twice
  long long frame_bytes;     // W*H*stride
  long long fres_size;       // rows*row_block
};

// Per-batch device workspace of the encoder. Every array is indexed
// [frame][...] with the stated per-frame stride (in elements).
struct EncWs {
  uint8_t *avg, *low;        size_t plane_stride;  // C*rows*cols (padded)
  uint8_t *lres_sym;         size_t lres_stride;
  uint8_t *fres_sym;         size_t fres_stride;
  uint32_t *hist;            // [f][2][kHistStride]      0 = LRES, 1 = FRES
  uint32_t *span_hist_l;     // [f][lres_spans][kHistStride]
  uint32_t *span_hist_f;     // [f][rows][kHistStride]
  uint32_t *lres_trail;      // [f][lres_spans]  trailing zeros | allzero<<31
  uint64_t *codes;           // [f][2][kHistStride]
  uint32_t *lens;            // [f][2][kHistStride]
  uint8_t *tree;             // [f][2][kTreeStride]
  uint32_t *tree_nbytes;     // [f][2]
  uint64_t *span_bit0;       // [f][lres_spans + rows] absolute start bit in the frame's output
  uint32_t *span_bits;       // [f][lres_spans + rows] payload bits of the span
  int32_t *status;           // [f]
  // Token stream of the FRES rows (k_tok -> k_emit_tok; nullptr: k_tok_hist / k_emit_t work on the dense symbol plane).
  // A block row is cut into tok_nseg segments of tok_seg symbols; segment s of row r of frame f owns
  // tok_cap 16-bit slots at tok + ((f * rows + r) * tok_nseg + s) * tok_cap and its slot count
  // (a multiple of 8 slots is always written: the tail is padded with no-op slots) in tok_cnt.
  uint16_t *tok;
  uint32_t *tok_cnt;         // [f][rows][tok_nseg]
  int tok_seg, tok_nseg, tok_cap;
};

// Token slots (16 bits; see k_tok): literal | zeros in front << 8 (literal 1..255, 0..255 zeros);
// 0 = no-op; a run of zeros on its own takes an even-aligned pair of slots: kTokRunMark, then its length.
constexpr uint32_t kTokRunMark = 0x0100u;
constexpr int kTokMaxRun = 255;          // zeros a literal slot can carry
constexpr int kTokIter = 2048;           // symbols per wavefront iteration of the tokeniser (32 per lane)
constexpr int kTokRunPiece = 16662;      // zeros of one run on its own (the reference's greedy split: three slots each)
constexpr int kTokStage = 1152;          // slots of a wavefront's staging buffer in k_tok (2.25 KiB: eight workgroups per CU)
// How many slots a stretch of n symbols of a row can need, whatever the row holds.  Its slots are
// L + 3 P: L non-zero symbols, P pieces of runs on their own.  Such a run is a lead of more than
// 255 zeros in front of a literal of the stretch, or the row's trailing zeros (at least one).
//   * A lead that began in front of the stretch (at most one) costs the stretch no symbol; every
//     other lead has its 256 zeros and more inside, the trailing run at least one: with k and t of
//     them L <= n - 256 k - t, and the R <= 1 + k + t runs give L + 3 R <= n + 3 - 253 k + 2 t <= n + 5.
//   * A run of z zeros is ceil(z / 16662) <= 1 + floor(z / 16662) pieces, the runs are disjoint and
//     runs never cross block rows: P <= R + floor(Z / 16662), Z <= row_block the zeros they cover.
// So the stretch needs at most n + 5 + 3 floor(row_block / 16662) slots (tests/tok_model.py counts
// them by k_tok's rules; tests/test_tok_capacity.py holds the two against each other).
inline int tok_slots_beyond(int zeros_max) { return 5 + 3 * (zeros_max / kTokRunPiece); }
// Slots a segment owns beyond its symbol count: that bound, whole 16-byte pieces (the tail of a
// segment is padded to one); never less than the 64 every row below 333 240 symbols had before.
inline int tok_seg_pad(int row_block) {
  const int pad = (tok_slots_beyond(row_block) + 7) & ~7;
  return pad > 64 ? pad : 64;
}
// Slots k_tok can have in a wavefront's stage at once.  An iteration that fits with what is
// carried over is staged whole (the split test); otherwise half by half: n = 1024 symbols and
// c < 8 slots carried over from the segment's earlier symbols.  c > 0 means the segment has a
// non-zero symbol in front of the half, so every run the half emits lies inside the segment.
inline int tok_stage_need(int row_block, int seg) {
  const int alone = 1024 + tok_slots_beyond(row_block);
  const int carried = 7 + 1024 + tok_slots_beyond(seg < row_block ? seg : row_block);
  return alone > carried ? alone : carried;
}

// Container bytes that do not depend on the pixel data, built on the host.
struct StaticChunks {
  uint8_t head[176];  // RIFF..HIMG FRMT LMAP 'LRES' <size>   (kHeadLen bytes)
  uint8_t mid[272];   // QCFG FMAP 'FRES' <size>
  int mid_len;        // 268 with chroma table, 236 without
};

struct ShiftTables {
  uint8_t s[2][64];  // [0] luma, [1] chroma; row-major coefficient position
};

struct LresTables {
  int16_t tab[128];   // low-res companding table (positive half)
  uint8_t code[512];  // code[delta + 255] for delta in [-255, 255]
};

// Everything of the encoder that depends on the quality, for ONE quality (encode with a quality per
// frame, encode to a byte budget): a context holds 101 of them in HBM, and the quality-indexed
// forms of the kernels read entry quality[frame] where the others read their kernel arguments.
struct QualTab {
  uint32_t pq[3][2][64];  // the pixel stage's quantiser words (PixQuant: rr, kk, ss x luma / chroma x scan position)
  ShiftTables st;
  LresTables lt;
  uint8_t lmap[128];      // the LMAP chunk's payload (StaticChunks::head + 39)
  uint8_t qcfg[64];       // the QCFG chunk's payload, luma then chroma (StaticChunks::mid + 8; 32 bytes without chroma)
};
constexpr int kQualities = 101;
struct QualSel {
  const QualTab *tab;       // [kQualities]
  const int32_t *quality;   // [frame], each in [0, 100]
};

// A window per frame of pitched source pictures (himg_hip_encode_windows_device): frame f of the
// launch is the w x h picture (Geom::W, H) whose first pixel is at
// base + f * frame_pitch + y_f * row_pitch + x_f * Geom::stride, its rows row_pitch bytes apart.
struct WinSrc {
  const uint8_t *base;
  size_t row_pitch, frame_pitch;   // frame_pitch 0: every window of one picture
  const int32_t *org;              // [frame][x_f, y_f], on the device, checked by the host
};

// ---- decoder ---------------------------------------------------------------

constexpr int kLutBits = 11;  // width of the Huffman decode group table
constexpr int kDecThreads = 1024;
constexpr int kSubEntries = 1024;  // second-level decode table (codes longer than kLutBits)
constexpr int kSubMaxBits = 6;     // widest second-level sub-table
constexpr int kLresSubBits = 256;  // parallel LRES decode: payload bits per lane of a chunk (kDecThreads lanes)

struct DecStream {           // one Huffman stream (LRES or FRES) of one frame
  uint32_t payload_off;      // byte offset (in the packed stream) after the aligned tree
  uint32_t chunk_end;        // byte offset of the end of the chunk
  int32_t root;              // node index of the root
  int32_t num_nodes;
};

struct DecFrame {            // written by k_dec_parse, read by later kernels
  int32_t status;
  int32_t parse_status;      // k_dec_parse's own verdict (status collects the later kernels' as well)
  int32_t walk_status;       // k_dec_rowwalk's verdict: it runs beside k_dec_parse, k_row_count merges it
  uint32_t rows_first;       // k_dec_rowwalk: byte offset of the first FRES row header (0: not found)
  uint32_t walk_q, walk_r, walk_end;   // k_dec_rowwalk in several launches: where the next one resumes (walk_q 0: finished)
  int32_t ycbcr;
  DecStream s[2];
  int16_t lmap[128];         // decoder-side companding tables (positive halves)
  int16_t fmap[128];
  uint8_t shift[2][64];
  // The row kernels' small tables, the same for every block row of the frame -- built once by
  // k_dec_parse, copied (kRowTabWords / 4 x 16 bytes) by every row workgroup: the code byte ->
  // dequantised magnitude (int16 [256]), the shifts (u8 [2][64]), the shifts as packed pairs in
  // tile_plane's register order (u32 [2][32]) and the identity-test words (u32 [4]).
  alignas(16) uint32_t row_tabs[128 + 32 + 64 + 4];
};
constexpr int kRowTabWords = 128 + 32 + 64 + 4;
static_assert(kRowTabWords % 4 == 0, "whole 16-byte words");

constexpr int kLresMemoWords = 6;
// Header words behind a row's kDecThreads lane offsets (lane_off): [0] symbols of the row,
// [1] where the chain ends (bits), [2] valid flag, [3] diagnostics, [4] 1: lane_q holds
// three more boundaries inside every lane's range (wide rows), [8 + w] the QUARTER record
// (4 * lane + k) that holds the first symbol of window w of the row's symbols (w >= 1).
constexpr int kRecHdr = 72;
constexpr int kRecWin = 8;
struct DecWs {
  DecFrame *frames;          // [f]
  uint32_t *nodes;           // [f][2][522]  child a | child b << 10 | (symbol + 1) << 20 (1023: no child; 0: a branch)
  uint2 *grp;                // [f][2][1<<kLutBits] group table (kernels_dec.hip GrpTables)
  uint32_t *gyc;             // [f][2][1<<kLutBits] step words of the count-only groups (no four-byte limit)
  uint2 *sub;                // [f][2][kSubEntries] second-level entries for codes longer than kLutBits (.x byte / node, .y step word)
  uint32_t *row_off;         // [f][rows] payload byte offset of each FRES row
  uint32_t *row_len;         // [f][rows]
  uint8_t *lres_sym;         size_t lres_stride;
  uint8_t *fres_sym;         size_t fres_stride;
  uint8_t *low;              size_t plane_stride;
  // k_row_count -> k_dec_row_fused: per FRES row and lane the first owned token
  // (bits from the chunk start) and the exclusive prefix of the symbol counts.
  uint32_t *lane_start;      // [f][rows][kDecThreads]
  uint32_t *lane_off;        // [f][rows][kDecThreads + kRecHdr]: offsets, then total, chain end (bits), valid flag
                             // (1: the lanes' ranges are divided at token boundaries and a consumer finishes its
                             // range token by token; 3: k_row_count_w -- at boundaries of the WRITE pass's chain
                             // of groups: a consumer that walks those groups from its start lands on its limit)
  // Rows too wide for the LDS (k_row_window): three more boundaries inside every lane's range,
  // so that a 128 KiB window of the row's symbols has 1024 sub-sequences to walk, not 256.
  uint32_t *lane_q;          // [f][rows][6][kDecThreads]: positions of the boundaries at 1/4, 1/2, 3/4 (bits from the
                             // row's first), then the output offsets there; nullptr for rows the fused kernel takes
  uint32_t *parse_stats;     // [f][4] k_dec_parse phase cycles / 16
  uint32_t *stats;           // [f][rows+1][8] k_dec_huff counters (chunks, rounds, cycle splits)
  uint32_t *rc_stats;        // [f][rows][8] k_row_count phase cycles / 16 (slowest wave)
  // Parallel LRES decode (k_lres_spec / verify / write).
  int lres_chunks;           // chunk slots per frame (upper bound from lres_size)
  uint32_t *spec_start;      // [f][lres_chunks][1024] lane start, bits from the chunk's nominal start
  uint32_t *spec_endpos;     // [f][lres_chunks][1024] lane end, same origin
  uint32_t *spec_cnt;        // [f][lres_chunks][1024] symbols per lane
  uint32_t *spec_memo;       // [f][lres_chunks][1024][kLresMemoWords] starts the lane has decoded from, packed
  uint64_t *spec_end;        // [f][lres_chunks] payload bit where the chunk's speculative chain ends
  uint64_t *fix_end;         // [f][lres_chunks] the same after the correction pass
  uint64_t *spec_tot;        // [f][lres_chunks] symbols of the chunk
  uint64_t *ver_base;        // [f][lres_chunks] output offset of the chunk
  int32_t *ver_ok;           // [f] 1 when every chunk verified
  uint64_t *lres_endbit;     // [f] bits consumed when the LRES output became complete
};

// ---- launch wrappers (defined in kernels_enc.hip / kernels_dec.hip) --------

struct Profiler;  // host-side, see himg_hip.hip

// Does launch_encode tokenise the FRES rows into slots (and so need EncWs::tok) for this call?
bool enc_uses_row_tokens(const Geom &g, int batch);
// Symbols per token segment for this geometry (a multiple of kTokIter).
int enc_tok_seg(const Geom &g);
// Can k_tok take this geometry's rows at all (half an iteration's slots fit a wavefront's stage)?
inline bool enc_tok_stage_fits(const Geom &g) { return tok_stage_need(g.row_block, enc_tok_seg(g)) <= kTokStage; }
// Debug: expand frame `frame`'s token stream into symbols again (dst: fres_size bytes).
void launch_tok_expand(const Geom &g, const EncWs &ws, int frame, uint8_t *dst, hipStream_t stream);

// Debug: k_tree alone over both stream slots of n frames (only hist, codes, lens, tree, tree_nbytes and
// status of ws are touched: himg_hip_debug_trees).
void launch_debug_trees(const EncWs &ws, int n, hipStream_t stream);

void launch_encode(const Geom &g, const EncWs &ws, int batch, const uint8_t *d_frames,
                   uint8_t *d_out, size_t out_stride, uint32_t *d_sizes,
                   const StaticChunks &sc, const ShiftTables &st, const LresTables &lt,
                   const uint8_t *d_fmap_lut, hipStream_t stream, Profiler *prof,
                   hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join);

// One quality's entry of the table, from what build_static makes for that quality (host).
void enc_fill_qual_tab(const StaticChunks &sc, const ShiftTables &st, const LresTables &lt, QualTab *qt);
// launch_encode with frame f's tables taken from qs.tab[qs.quality[f]] (sc: build_static's for any
// quality; its LMAP / QCFG payloads are not used).  d_out == nullptr: the size-only pass -- everything
// up to k_span_bits, then the sizes alone to d_sizes: no byte of a stream is written, out_stride is
// not looked at, and only the histograms and status words are zeroed in front of it.
void launch_encode_q(const Geom &g, const EncWs &ws, int batch, const uint8_t *d_frames,
                     uint8_t *d_out, size_t out_stride, uint32_t *d_sizes,
                     const StaticChunks &sc, const QualSel &qs,
                     const uint8_t *d_fmap_lut, hipStream_t stream, Profiler *prof,
                     hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join);
// launch_encode_q with frame f read from its window of src (g: the windows' geometry).
void launch_encode_windows(const Geom &g, const EncWs &ws, int batch, const WinSrc &src,
                           uint8_t *d_out, size_t out_stride, uint32_t *d_sizes,
                           const StaticChunks &sc, const QualSel &qs,
                           const uint8_t *d_fmap_lut, hipStream_t stream, Profiler *prof,
                           hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join);
// The quality searches of himg_hip_encode_budget_device and himg_hip_encode_target_device, per frame on
// the device: a SearchFrame (search_step.h) per frame, one array per field.
struct SearchState {
  int32_t *quality;          // (first in the buffer: the per-quality forms keep their QualSel::quality there)
  uint64_t *limit, *best;
  uint64_t *value;           // [f] where a probe with 64-bit values leaves them (the distortion probe's sums)
  int32_t *ok, *bad, *state, *err;
};
// The buffer behind a SearchState -- these two alone know its layout: the qualities (an even number of
// words), the 64-bit arrays, the other words.  The qualities and the limits are adjacent: one copy stages both.
inline size_t search_state_bytes(int batch) { return ((((size_t)batch + 1) & ~(size_t)1) + 10 * (size_t)batch) * 4; }
inline SearchState search_state_carve(void *base, int batch) {
  const size_t b = (size_t)batch;
  int32_t *w = (int32_t *)base;
  uint64_t *d = (uint64_t *)(w + ((b + 1) & ~(size_t)1));
  int32_t *t = (int32_t *)(d + 3 * b);
  return SearchState{w, d, d + b, d + 2 * b, t, t + b, t + 2 * b, t + 3 * b};
}
// Behind probe `probe` of `probes`: search_step for every frame, the probe's values from d_sizes, or
// from ss.value when that is null.  The last one leaves quality[f] = the result (qmin for a frame
// without one) and d_quality[f] (-1).
void launch_search_step(const SearchState &ss, const EncWs &ws, int batch, int probe, int probes, int dir, int qmin,
                        int qmax, const uint32_t *d_sizes, int32_t *d_quality, hipStream_t stream, Profiler *prof);
// Behind the final encode: d_status[f] (the encode's own, or the search's failure: miss_code for a frame
// whose first probe missed its limit, else the failed probe's status) and d_sizes[f] = 0 for a failed
// frame; d_sse (may be null): the value at the chosen quality, at the first probe's for a miss, 0 after an error.
void launch_search_finish(const SearchState &ss, const EncWs &ws, int batch, int miss_code, uint32_t *d_sizes,
                          uint64_t *d_sse, int32_t *d_status, hipStream_t stream, Profiler *prof);

// ---- the distortion probe (himg_hip_encode_sse_device, himg_hip_encode_target_device) ----
// The decode-side tables of a stream of ONE quality, as k_dec_parse builds DecFrame::row_tabs from
// the stream's FMAP and QCFG chunks: the code byte -> dequantised magnitude (int16 [256]), the shifts
// (u8 [2][64]), the shifts as packed pairs in tile_plane's register order (u32 [2][32]) and the
// identity-test words (u32 [4]).  A context holds kQualities of them in HBM beside the QualTab's.
struct SseTab {
  alignas(16) uint32_t w[128 + 32 + 64 + 4];
};
void sse_fill_tab(const int16_t fmap[128], const ShiftTables &st, SseTab *t);   // (host)
struct SseArgs {
  uint8_t *rec;          // [f] the reconstructed low-res plane, [C][rows][cols], EncWs::plane_stride apart
  const SseTab *tab;     // [kQualities]
  uint64_t *sse;         // [f] the result
};
// k_sse (kernels_dec.hip, beside the inverse transform it shares): frame f's symbols in ws.fres_sym
// through the decoder's inverse path at quality qs.quality[f], compared with the source; the sums
// are ADDED to sa.sse[f] (zeroed by the caller).
void launch_sse(const Geom &g, const EncWs &ws, int batch, const uint8_t *d_frames, const QualSel &qs,
                const SseArgs &sa, hipStream_t stream, Profiler *prof);
// The probe's launch sequence: launch_encode_q's front (k_front, or the averages, the blend and the
// pixel / tile stage), the low-res chain in the form that stores its reconstructed samples, k_sse.
void launch_encode_sse(const Geom &g, const EncWs &ws, int batch, const uint8_t *d_frames,
                       const StaticChunks &sc, const QualSel &qs, const SseArgs &sse,
                       const uint8_t *d_fmap_lut, hipStream_t stream, Profiler *prof,
                       hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join);

// The decoder's helper streams and events (owned by the context).
constexpr int kWalkSegs = 4;   // single large frames: at most this many row ranges whose walk / count / row kernels overlap
struct DecStreams {
  hipStream_t side = nullptr;    // the serial row-header walk; k_row_count behind it (batches)
  hipStream_t side2 = nullptr;   // single frames: k_row_count of a row range while `side` walks the next one
  hipStream_t side3 = nullptr;   // rows wider than the LDS: the entropy pass of a row range (k_row_window) while
                                 // `side2` counts the next one and the caller's stream runs the LRES chain / transforms
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_walk[kWalkSegs] = {}, ev_cnt[kWalkSegs] = {}, ev_win[kWalkSegs] = {};
};

// What of a context's settings only the host's launch code reads (what the kernels read goes
// through Geom).  Set once, when the context is created.
struct HostOpts {
  bool allow_fused = true;   // HIMG_FORCE_UNFUSED=1: every block row through the generic decode path
  bool use_side = true;      // HIMG_SIDE_STREAM=0: no side streams (decoder and encoder)
  int walk_segs = 0;         // HIMG_WALK_SEGS: row ranges of a single frame's decode (0: by frame size)
  int persist_rows = 1;      // HIMG_PERSIST_ROWS: persistent row workgroups (1: one per CU; 0: off; n > 1: n)
  int n_cu = 256;            // compute units of the context's device
};

// The fused row kernel serves this geometry (a block row's symbols and the decode tables fit
// the LDS of one CU); otherwise the rows go through 128 KiB windows (k_row_window).
bool dec_rows_fit_lds(const Geom &g);
constexpr int kLoopCounters = 8;
// Loop trip counters of a -DHIMG_LOOP_COUNTS build (loop_counts.h): read and reset; -1 when not compiled in.
int loop_counts_read_enc(unsigned long long *out);
int loop_counts_read_dec(unsigned long long *out);

// The planar float output (himg_hip_tensor_desc as the kernels take it): element (f, c, i, j) of
// [batch][co][H][W] is cvt(fma((float)p, scale[c], bias[c])) of byte (i, j, c) of the uint8 picture.
// It travels in the kernel-argument segment of the tensor forms of the store kernels
// (k_dec_row_fused_t, k_tile_inv_t, k_dec_region_t), which read scale / bias there at their use.
struct TensDesc {
  int dtype, co;   // HIMG_DT_*; the first co channels are stored
  float scale[4], bias[4];
};
__host__ __device__ inline int tens_elem_size(int dtype) { return dtype == 0 ? 4 : 2; }

// The pitched destination (himg_hip_dst as the kernels take it): pixel (i, j), channel c of frame f's
// decoded picture -- or of its window, for the region decode -- is the byte at
//   d_out + f * frame_pitch + (org[2 f + 1] + i) * row_pitch + (org[2 f] + j) * pixel_stride + c.
// It travels in the kernel-argument segment of the pitched forms of the store kernels
// (k_dec_row_fused_p, k_tile_inv_p, k_dec_region_p), which read the pitch and the stride there at
// their stores; org is on the device, behind the packed sizes (and the region decode's own origins).
struct DstDesc {
  size_t row_pitch, frame_pitch;
  const int32_t *org;
  int pixel_stride;
};

// The picture pyramid (himg_hip_pyramid as the kernels take it): level[k] is the picture at 1 / 2^k,
// batch x ceil(H / 2^k) x ceil(W / 2^k) x C interleaved bytes, frame f at f * oh * ow * C; nullptr: the
// level is not wanted and nothing of it is computed or stored.  It travels in the kernel-argument
// segment of the pyramid forms of the store kernels (k_dec_row_fused_m, k_tile_inv_m), which read
// the pointers there, behind the entropy phase.
struct PyrDesc {
  uint8_t *level[4];
};

// The stream's own planes (himg_hip_decode_planes_device): bit c of mask set for each wanted channel c
// of the stream, P = popcount(mask) planes per frame in ascending channel order, frame f's [P][H][W]
// bytes at f * P * H * W.  Plane c holds the bytes in front of the colour inverse, which never runs.
// It travels in the kernel-argument segment of the planes forms of the store kernels
// (k_dec_row_fused_c, k_tile_inv_c), which read the mask there: in front of the transform -- an
// unselected channel's tile_plane is not run -- and at the stores.
struct PlaneDesc {
  uint32_t mask;
};
__host__ __device__ inline int plane_count(uint32_t mask) {
  return (int)((mask & 1u) + ((mask >> 1) & 1u) + ((mask >> 2) & 1u) + ((mask >> 3) & 1u));
}

// The form in which the pixel-writing kernels store: interleaved uint8 (no descriptor), or one of the
// four forms above with its descriptor, which the launch copies into the kernel's arguments.
enum StoreKind { kStoreU8, kStoreTens, kStorePitch, kStorePyr, kStorePlanes };
struct StoreForm {
  StoreKind kind = kStoreU8;
  const void *desc = nullptr;   // the kind's descriptor
  StoreForm() = default;
  StoreForm(const TensDesc *t) : kind(kStoreTens), desc(t) {}
  StoreForm(const DstDesc *d) : kind(kStorePitch), desc(d) {}
  StoreForm(const PyrDesc *m) : kind(kStorePyr), desc(m) {}
  StoreForm(const PlaneDesc *c) : kind(kStorePlanes), desc(c) {}
  const TensDesc &tens() const { return *static_cast<const TensDesc *>(desc); }
  const DstDesc &dst() const { return *static_cast<const DstDesc *>(desc); }
  const PyrDesc &pyr() const { return *static_cast<const PyrDesc *>(desc); }
  const PlaneDesc &planes() const { return *static_cast<const PlaneDesc *>(desc); }
};

// form: kStoreTens, the pixel-writing kernels run in their tensor form (d_out: [batch][co][H][W]
// elements); kStorePitch: in their pitched form (d_out: the destination pictures); kStorePyr: in their
// pyramid form (d_out: level[0], which may be nullptr; level 3 is k_lres_preview's, behind the LRES
// chain); kStorePlanes: in their planes form (d_out: [batch][P][H][W] bytes).  Everything in front of
// them is the same launch.
void launch_decode(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed,
                   size_t in_stride, const uint32_t *d_sizes, uint8_t *d_out,
                   int32_t *d_status, hipStream_t stream, Profiler *prof, const HostOpts &ho,
                   const DecStreams *ds, int r0, int r1,
                   const uint32_t *d_row_index = nullptr, bool index_only = false, int phase = 3,
                   const StoreForm &form = StoreForm());
constexpr int kDecHead = 1, kDecRows = 2;   // launch_decode's phases
// The front of launch_decode's rows and no more (himg_hip_debug_row_records): container parse, row-header
// walk, then k_row_count_w over every row in the form g.count_stretch asks for.  No row kernel runs.
void launch_row_records(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                        const uint32_t *d_sizes, int32_t *d_status, hipStream_t stream, Profiler *prof);
// The 1/8-scale preview: the zeroing of the LRES symbols, the container parse up to the end of
// the LRES chunk (k_dec_parse_head, which writes where that chunk ends to d_head_sizes[f]), the
// LRES chain bounded there, the predictor inverse, then k_lres_preview: batch x ceil(H/8) x
// ceil(W/8) x C interleaved bytes at d_out; the verdict per frame to d_status.  Needs of the
// workspace only frames, the LRES stream's tables, lres_sym, low, stats and the spec_* scratch.
void launch_preview(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                    const uint32_t *d_sizes, uint32_t *d_head_sizes, uint8_t *d_out, int32_t *d_status,
                    hipStream_t stream, Profiler *prof);
// The region decode (scale_log2 = 0, k_dec_region): the window w x h at frame f's own origin
// (x_f, y_f) = org[2 f], org[2 f + 1] (h_org on the host, d_org the same on the device, both in range),
// every frame of the batch.  The head phase of the full decode (zeroing, k_dec_parse, the LRES chain),
// each frame's row index up to its block row r1_f = ceil((y_f + h) / 8) (d_row_index: given for
// rows [y_f / 8, r1_f) of each frame at 2 f rows words, k_region_set_index; else k_region_rowwalk
// stopping there, or walking on to the end of the chunk when r1_f is the last row; on ds->side
// beside the head phase when ds is given), the counts of each frame's rows [y_f / 8, r1_f), then
// the region kernel: batch x h x w x C interleaved bytes at d_out (frame f at f h w C).  No FRES
// symbol plane, no quarter records.
// The scaled region decode (scale_log2 = 1, 2, k_dec_scaled_region): the window w x h of the picture
// at 1 / 2^scale_log2, frame f's window at its own origin (x_f, y_f) in that picture.  h_org / d_org:
// the origins of the full-resolution rectangles the windows cover, (F x_f, F y_f), F = 2^scale_log2 --
// what the walk and count kernels take, here with the height F h; the caller has checked
// x_f + w <= ceil(W / F) and y_f + h <= ceil(H / F).  The same head phase, walk and counts, then the
// scaled kernel over the touched block rows and tile columns.
void launch_region(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                   const uint32_t *d_sizes, const uint32_t *d_row_index, const int32_t *h_org, const int32_t *d_org,
                   int scale_log2, int w, int h, uint8_t *d_out, int32_t *d_status, hipStream_t stream, Profiler *prof,
                   const DecStreams *ds,
                   const StoreForm &form = StoreForm());   // (scale_log2 = 0 only: kStoreTens, [batch][co][h][w]; kStorePitch, windows of the pictures)
// Many windows of one stream (include/himg_hip.h, himg_hip_decode_stream_regions_device): window k, the
// w x h rectangle at (org[2 k], org[2 k + 1]) of stream stream_of[k], to d_out + k h w C and d_status[k].
// The head phase runs once per stream; the walk once per stream, to row_end[s] (the largest r1_k of its
// windows, 0x7fffffff to the end of the chunk where one reaches the last block row, 0 for a stream no window
// names) -- or, with d_row_index, the host's index of rows [index_rows[2 s], index_rows[2 s + 1]) --; the
// counts run over list, n_list entries (stream, first row, end row) of at most stream_count_chunk() rows,
// every touched (stream, row) once; the row kernel over (strip, row, window).  The words are device
// pointers, staged by the caller behind the packed sizes; scratch: 2 n_streams + n_windows words.  h_org:
// the origins on the host.  The workspace of launch_region.
struct StreamRegionWords {
  const int32_t *stream_of, *org, *row_end, *list, *index_rows;
  int32_t *scratch;
};
int stream_count_chunk(const Geom &g, long long list_rows);
void launch_stream_regions(const Geom &g, const DecWs &ws, int n_streams, const uint8_t *d_packed, size_t in_stride,
                           const uint32_t *d_sizes, const uint32_t *d_row_index, const StreamRegionWords &d_words,
                           int n_windows, const int32_t *h_org, int n_list, long long list_rows, int w, int h,
                           uint8_t *d_out, int32_t *d_status, hipStream_t stream, Profiler *prof, const DecStreams *ds);
// Opened streams (include/himg_hip.h, himg_hip_open_streams_device): the head of launch_stream_regions once per
// stream with the walk over ALL its row headers (d_row_index: the host's index of all rows instead), its
// products written through ws -- the HANDLE's frames, tables, row index, low-res planes, records and counters,
// with the context's LRES scratch (lres_sym, spec_*) beside them --, every record's valid word cleared, the
// head verdicts to d_head_status (may be null).  walk: n_streams words each, the handle's.
struct OpenedWalk {
  int32_t *rows, *st;   // k_stream_rowwalk's walk_rows / walk_st of a walk to the end of the chunk
};
void launch_open_streams(const Geom &g, const DecWs &ws, int n_streams, const uint8_t *d_packed, size_t in_stride,
                         const uint32_t *d_sizes, const uint32_t *d_row_index, const OpenedWalk &walk,
                         int32_t *d_head_status, hipStream_t stream, Profiler *prof, const DecStreams *ds);
// A call on the handle (himg_hip_opened_regions_device): launch_stream_regions' gate, counts and row kernel
// and nothing in front of them.  d_list: n_list entries over the list_rows rows that no earlier call has
// counted (opened_plan.h), n_list = 0: no count kernel runs.  d_status doubles as the windows' own words.
void launch_opened_regions(const Geom &g, const DecWs &ws, const uint8_t *d_packed, size_t in_stride,
                           const uint32_t *d_sizes, const OpenedWalk &walk, const int32_t *d_stream_of,
                           const int32_t *d_org, const int32_t *d_list, int n_windows, const int32_t *h_org, int n_list,
                           long long list_rows, int w, int h, uint8_t *d_out, int32_t *d_status, hipStream_t stream,
                           Profiler *prof);
// A scaled call on the handle (himg_hip_opened_scaled_regions_device): window k, w x h samples of stream
// stream_of[k]'s picture at 1 / 2^scale_log2.  scale_log2 = 1, 2: h_org / d_org hold the origins of the
// full-resolution rectangles the windows cover, (F x_k, F y_k), as launch_region takes them; k_opened_gate and the
// counts over d_list run with the height F h -- the list is the handle's, so a row counted by a full-resolution
// call is not counted again, and the other way round --, then k_dec_opened_scaled_region.  scale_log2 = 3: d_org
// holds the origins in the ceil(W / 8) x ceil(H / 8) picture; k_opened_preview_region alone crops the kept
// low-res plane and writes the kept head verdict; d_list, h_org and d_packed are not used.
void launch_opened_scaled_regions(const Geom &g, const DecWs &ws, const uint8_t *d_packed, size_t in_stride,
                                  const uint32_t *d_sizes, const OpenedWalk &walk, int scale_log2,
                                  const int32_t *d_stream_of, const int32_t *d_org, const int32_t *d_list, int n_windows,
                                  const int32_t *h_org, int n_list, long long list_rows, int w, int h, uint8_t *d_out,
                                  int32_t *d_status, hipStream_t stream, Profiler *prof);
// The decode of stream prefixes (include/himg_hip.h): frame f's first d_words[f] bytes are present.
// k_span_gate (the head of the stream with every load checked against the bytes present, then the frame's
// state against what it found), the head phase in its prefix form (k_dec_parse_prefix, the LRES chain
// bounded by the bytes present), k_span_rowwalk beside it (ds given: on ds->side) -- the row index and k_f,
// the rows that are whole --, k_prefix_fill for rows [k_f, rows), the count kernels and k_dec_region's body
// (k_dec_span) over the rows to decode.  d_state == nullptr: those are rows [0, k_f) of every frame.  Else
// the prefix decode continued (himg_hip_decode_prefix_more_device): d_state holds a PfxState (prefix_walk.h)
// per frame, read and -- for a frame without a verdict -- advanced on the device.  A fresh state's frame is
// decoded as without states; of a resumed one only block rows [rows_done, k_new) are walked, counted, decoded
// and stored, and nothing else of its picture is written.  d_words: 8 x batch words, the first batch staged
// by the caller; d_rows: k_f, or -1 with a verdict.  The workspace of launch_region.
struct PfxState;
void launch_prefix(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                   uint32_t *d_words, PfxState *d_state /* may be null */, uint8_t *d_out, int32_t *d_rows,
                   int32_t *d_status, hipStream_t stream, Profiler *prof, const DecStreams *ds);
// The concealing decode (include/himg_hip.h): launch_decode as himg_hip_decode_device calls it, into d_out, then
// the repair pass over the frames it rejected in their FRES rows alone (kernels_dec.hip, k_conceal_gate ..
// k_conceal_status), on the caller's stream with no host wait.  d_words: 5 x batch words, the first batch --
// the packed sizes -- staged by the caller; d_cmap: batch x rows bytes of scratch; d_rowmap may be nullptr.
// The workspace of launch_decode (the repair pass writes plain per-lane records over the full decode's).
void launch_conceal(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                    uint32_t *d_words, uint8_t *d_cmap, uint8_t *d_out, int32_t *d_concealed, uint8_t *d_rowmap,
                    int32_t *d_status, hipStream_t stream, Profiler *prof, const HostOpts &ho, const DecStreams *ds);
// Widest column strip of the region kernel, in tiles (its LDS holds C x 64 segments of a strip).
int region_strip_tiles(const Geom &g);
// The scaled decode (k_dec_scaled): every frame of the batch at 1 / 2^scale_log2 (1 or 2) of its
// size from the S x S lowest-sequency coefficients of every tile (S = 8 >> scale_log2; the
// definition: include/himg_hip.h).  The head phase, the row walk and the count kernels are the
// full decode's (every row one record, as in launch_region); d_row_index: the host's index of
// one frame (batch == 1).  batch x ceil(H / F) x ceil(W / F) x C interleaved bytes at d_out.
// No FRES symbol plane, no quarter records.
void launch_scaled(const Geom &g, const DecWs &ws, int batch, const uint8_t *d_packed, size_t in_stride,
                   const uint32_t *d_sizes, const uint32_t *d_row_index, int scale_log2, uint8_t *d_out,
                   int32_t *d_status, hipStream_t stream, Profiler *prof, const DecStreams *ds);
// Widest column strip of the scaled kernel, in tiles (its LDS holds C x S x S segments of a strip).
int scaled_strip_tiles(const Geom &g, int scale_log2);
// The row-header walk of one frame alone (row-sharded decode: beside the head phase).
void launch_rowwalk_only(const Geom &g, const DecWs &ws, const uint8_t *d_packed, size_t in_stride,
                         const uint32_t *d_sizes, hipStream_t stream);
// ... up to (not including) block row `row_end`; resume: go on where the launch before stopped.
void launch_rowwalk_range(const Geom &g, const DecWs &ws, const uint8_t *d_packed, size_t in_stride,
                          const uint32_t *d_sizes, int row_end, bool resume, hipStream_t stream);

// Row-sharded encode of one frame (multi-GPU): phases between the collectives.
void launch_shard_stats(const Geom &g, const EncWs &ws, const uint8_t *d_frame_base,
                        const ShiftTables &st, const uint8_t *d_fmap_lut, int r0, int r1,
                        hipStream_t stream, Profiler *prof);
void launch_shard_row_bits(const Geom &g, const EncWs &ws, int r0, int r1, uint32_t *d_bits_out,
                           hipStream_t stream, Profiler *prof);
void launch_shard_emit(const Geom &g, const EncWs &ws, const StaticChunks &sc,
                       const uint32_t *d_all_row_bits, uint8_t *d_rel, size_t rel_cap,
                       uint32_t *d_rel_size, int r0, int r1, hipStream_t stream, Profiler *prof);
void launch_shard_assemble(const Geom &g, const EncWs &ws, const StaticChunks &sc,
                           const LresTables &lt, const uint32_t *d_all_row_bits,
                           const uint8_t *d_rel, size_t rel_bytes, uint8_t *d_out, size_t out_cap,
                           uint32_t *d_size, hipStream_t stream, Profiler *prof);

void launch_shard_head(const Geom &g, const EncWs &ws, const StaticChunks &sc, const LresTables &lt,
                       const uint32_t *d_all_row_bits, uint8_t *d_out, size_t out_cap, uint32_t *d_size,
                       uint32_t *d_head, int r0, int r1, hipStream_t stream, Profiler *prof);
void launch_shard_finish(const Geom &g, const EncWs &ws, uint8_t *d_out, size_t out_cap, const uint32_t *d_size,
                         hipStream_t stream, Profiler *prof);

// The dynamic-LDS limits of the kernels that need more than the default, set on the current
// device (once per context, at creation).
hipError_t enc_set_kernel_attrs();
hipError_t dec_set_kernel_attrs();

// Stage timing hook: called before/after every kernel launch when profiling.
void prof_begin(Profiler *p, const char *stage, hipStream_t s);
void prof_end(Profiler *p, hipStream_t s);

}  // namespace himg_dev
#endif  // HIMG_DEV_H_
