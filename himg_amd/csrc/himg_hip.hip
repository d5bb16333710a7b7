// himg_hip.hip -- host side of the C ABI declared in include/himg_hip.h.
//
// Owns the device workspace, builds the data-independent container bytes and
// kernel tables on the host (they depend only on quality / geometry), and
// sequences the kernels of kernels_enc.hip / kernels_dec.hip.  There is no CPU
// fallback: every compute entry point needs a working HIP device.
#include "himg_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "himg_dev.h"
#include "himg_tables.h"
#include "opened_plan.h"
#include "prefix_walk.h"

using namespace himg_dev;

namespace himg_dev {

struct Profiler {
  bool enabled = false;
  struct Rec { const char *name; hipEvent_t a, b; };
  std::vector<Rec> pending;
  struct Acc { std::string name; double ms = 0; int n = 0; };
  std::vector<Acc> acc;
  const char *cur = nullptr;
  hipEvent_t cur_a = nullptr;

  void collect() {
    for (auto &r : pending) {
      hipEventSynchronize(r.b);
      float ms = 0;
      hipEventElapsedTime(&ms, r.a, r.b);
      hipEventDestroy(r.a);
      hipEventDestroy(r.b);
      size_t i = 0;
      for (; i < acc.size(); ++i)
        if (acc[i].name == r.name) break;
      if (i == acc.size()) { acc.push_back(Acc()); acc.back().name = r.name; }
      acc[i].ms += ms;
      acc[i].n += 1;
    }
    pending.clear();
  }
};

void prof_begin(Profiler *p, const char *stage, hipStream_t s) {
  if (!p || !p->enabled) return;
  p->cur = stage;
  hipEventCreate(&p->cur_a);
  hipEventRecord(p->cur_a, s);
}
void prof_end(Profiler *p, hipStream_t s) {
  if (!p || !p->enabled) return;
  hipEvent_t b;
  hipEventCreate(&b);
  hipEventRecord(b, s);
  p->pending.push_back({p->cur, p->cur_a, b});
}

}  // namespace himg_dev

namespace {

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  // Grow-only device allocation.
  bool reserve(size_t n) {
    if (n <= cap) return true;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, n) != hipSuccess) return false;
    cap = n;
    return true;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// What a host form reads back of a frame, as its device call writes it (the fields its form does not
// have stay unwritten) and as one copy fetches it.
struct HostResult {
  uint32_t size;
  int32_t status;
  int32_t quality;
  uint64_t sse;
};
// The batched host forms' pinned words: the mirrors of the two slots' results, and the packed sizes
// their decodes are handed.
struct PipeMeta {
  HostResult res[2];
  uint32_t dec_size[2];
};

}  // namespace

struct himg_hip_ctx {
  int device = 0;
  std::string err;
  Profiler prof;
  hipStream_t last_stream = nullptr;
  // Run-time settings: read from the environment once, in himg_hip_create; after that they
  // change only through himg_hip_set_option.  What the kernels read goes into every call's Geom
  // (apply_settings), what only the launch code reads is `opts`.
  HostOpts opts;
  int fix_t2 = 0;          // HIMG_OPT_FIX_T2 (or HIMG_FIX_T2=1 in the environment)
  int max_sub = 4096;      // HIMG_MAX_SUB_BITS: test knob, see Geom::max_sub
  int lead_bits = 128;     // HIMG_LEAD_BITS: tuning knob, see Geom::lead_bits
  int lres_serial = 0;     // HIMG_FORCE_LRES_SERIAL=1: test knob, see Geom::lres_serial
  int prefetch_rows = 1;   // HIMG_PREFETCH_ROWS: see Geom::prefetch_rows
  int count_wave = -1, emit_rows = -1;   // HIMG_OPT_COUNT_WAVE / _EMIT_ROWS (-1: by launch size)
  int count_stretch = -1;                // HIMG_OPT_COUNT_STRETCH (-1: the default)
  int row_tokens = -1;                   // HIMG_OPT_ROW_TOKENS (-1: by launch size)
  int front = -1;                        // HIMG_OPT_FRONT (-1: by launch size)
  // Side stream + events: the decoder forks its serial row-header walk onto it.
  DecStreams dstr;
  // The encoder's side stream carries its LRES branch, which is on the critical path
  // (k_tree waits for it): default priority, its own events -- not the decoder's
  // lowest-priority stream, behind whose wide k_row_count launches of other contexts it
  // would queue.
  hipStream_t side_enc = nullptr;
  hipEvent_t ev_fork_e = nullptr, ev_join_e = nullptr;

  // Fixed table: LUT of the full-res companding search (FullResMapper is the
  // same for every quality, mapper.cpp:213-223), 32769 entries.
  DevBuf fmap_lut;
  size_t host_bytes = 0;   // bytes of the last host-API result still resident in h_out
  // Batched host API: H2D of frame i+1, kernels of frame i and D2H of frame i-1 overlap
  // on three streams; staging is double buffered.
  struct Pipe {
    bool ready = false;
    hipStream_t s_in = nullptr, s_comp = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    DevBuf in[2], out[2], meta[2];     // meta: the frame's HostResult
    PipeMeta *h_meta = nullptr;        // pinned
  } pipe;

  // Encoder workspace.
  DevBuf e_planes, e_lres, e_fres, e_small, e_spanhist, e_tok, e_tokx;
  DevBuf e_dbgtree;          // himg_hip_debug_trees' scratch workspace
  // Quality per frame and the searches: the tables of all 101 qualities (built on first use) and
  // the per-frame words of a launch (a SearchState's arrays, the quality first).
  DevBuf e_qtab, e_search;
  // The distortion probe: the decode-side tables of all 101 qualities (built with e_qtab) and the
  // reconstructed low-res planes of a launch.
  DevBuf e_stab, e_rec;
  bool qtab_ready = false;
  Geom enc_geom{};
  EncWs enc_ws{};
  int enc_batch = 0;
  bool enc_valid = false;

  // Decoder workspace.
  DevBuf d_frames, d_nodes, d_grp, d_gyc, d_sub, d_lane, d_rows, d_lres, d_fres, d_planes, d_sizes, d_stats, d_spec;
  DevBuf d_cmap;   // the concealing decode's row map, [frame][rows] bytes
  Geom dec_geom{};
  DecWs dec_ws{};
  int dec_batch = 0;
  bool dec_valid = false;
  hipEvent_t ev_range[HIMG_MAX_WALK_RANGES] = {};   // himg_hip_decode_walk_ranges_device: behind every row range
  int n_ranges = 0;
  // What the last himg_hip_decode_head_device prepared (the frame tables and the low-res plane in
  // the decoder workspace): himg_hip_decode_rows_after_head_device must be handed the same
  // stream, geometry and HIP stream, with no other decode on this context in between (every
  // decode entry point goes through ensure_dec_ws, which drops the token).
  struct HeadToken {
    bool valid = false;
    int w = 0, h = 0, c = 0;
    const void *packed = nullptr;
    uint32_t size = 0;
    void *stream = nullptr;
  } head;

  // Staging for the host-buffer API.
  DevBuf h_in, h_out, h_result, h_status, h_index;   // h_result: a HostResult (encode); h_status: status words (decode)
  uint32_t *hp_index = nullptr;          // pinned staging of the host row index (stage_reserve)
  size_t hp_index_cap = 0;               // in dwords

  // Packed sizes handed to the decoder: the caller's array (or a by-value argument)
  // may be gone before an asynchronous copy reads it, so the sizes are first copied
  // into a ctx-owned pinned slot; a slot is reused only after the copy that read it
  // has run (event).
  struct SizeRing {
    static constexpr int kSlots = 8;   // (a viewer's open, pan and zoom calls queue behind one another without a wait)
    uint32_t *h[kSlots] = {};
    size_t cap[kSlots] = {};
    hipEvent_t ev[kSlots] = {};
    bool busy[kSlots] = {};
    int next = 0;
  } sizes_ring;

  // Row-sharded encode state (himg_hip_shard_*).
  struct {
    bool valid = false;
    Geom g{};
    StaticChunks sc{};
    ShiftTables st{};
    LresTables lt{};
    int r0 = 0, r1 = 0;
  } shard;

  // The opened-streams handles that belong to this context (himg_hip_open_streams_device); himg_hip_destroy
  // closes the ones that are left.
  std::vector<himg_hip_opened *> opened;
};

static int fail(himg_hip_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess) {
  if (ctx) {
    ctx->err = what;
    if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
  }
  return code;
}

#define HIP_TRY(ctx, expr)                                                  \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) return fail(ctx, HIMG_ERR_HIP, #expr, e_);        \
  } while (0)

static bool make_geom(int width, int height, int pixel_stride, int num_channels, int use_ycbcr,
                      Geom *g) {
  if (width < 1 || height < 1 || num_channels < 1 || num_channels > 4 ||
      pixel_stride < num_channels)
    return false;
  g->W = width; g->H = height; g->C = num_channels; g->stride = pixel_stride;
  g->rows = (height + 7) >> 3; g->cols = (width + 7) >> 3;
  g->mrows = (g->rows + 15) / 16; g->mcols = (g->cols + 15) / 16;
  g->chan_size = g->mrows * g->mcols + g->rows * g->cols;   // downsampled.cpp:171-175
  const long long lres = (long long)g->chan_size * num_channels;
  const long long fres = (long long)g->rows * g->cols * 64 * num_channels;
  // The reference keeps every size in `int` (encoder.cpp:81,270,339-341).
  if (fres > 0x7fffffffLL || (long long)width * height * pixel_stride > 0x7fffffffLL) return false;
  g->lres_size = (int)lres;
  g->row_block = g->cols * num_channels * 64;
  g->ycbcr = (use_ycbcr && num_channels >= 3) ? 1 : 0;   // encoder.cpp:69
  g->lres_spans = (g->lres_size + kLresSpan - 1) / kLresSpan;
  g->use_blocks = g->rows > 1 ? 1 : 0;                   // block_size < in_size
  g->fix_t2 = 0;
  g->max_sub = 4096;
  g->lead_bits = 128;
  g->lres_serial = 0;
  g->count_wave = g->emit_rows = g->row_tokens = g->front = -1;
  g->count_stretch = -1;
  g->wide_q = 0;
  g->prefetch_rows = 1;
  g->frame_bytes = (long long)width * height * pixel_stride;
  g->fres_size = fres;
  return true;
}

// The context's settings that kernels read, into the geometry of one of its calls.  Each
// kernel reads only its own side's: the encoder's emit_rows / row_tokens / front, the
// decoder's the rest -- and of those, the parse and row-header walk (all that the index, walk
// and first-header entries launch) read fix_t2 alone.
static void apply_settings(const himg_hip_ctx *ctx, Geom *g) {
  g->fix_t2 = ctx->fix_t2;
  g->max_sub = ctx->max_sub;
  g->lead_bits = ctx->lead_bits;
  g->lres_serial = ctx->lres_serial;
  g->prefetch_rows = ctx->prefetch_rows;
  g->count_wave = ctx->count_wave;
  g->count_stretch = ctx->count_stretch;
  g->emit_rows = ctx->emit_rows;
  g->row_tokens = ctx->row_tokens;
  g->front = ctx->front;
}

extern "C" size_t himg_hip_max_packed_size(int width, int height, int num_channels) {
  Geom g;
  if (!make_geom(width, height, num_channels, num_channels, 1, &g)) return 0;
  // Payloads never exceed their symbol counts by more than the tree
  // (huffman_enc.cpp:242-244 assumes the same); plus row headers and chunks.
  size_t n = 12 + 19 + 136 + 8 + 72 + 188 + 8;
  n += (size_t)g.lres_size + kTreeStride;
  n += (size_t)g.fres_size + kTreeStride + 4u * (size_t)g.rows;
  return round_up(n + 64, 256);
}

// HIMG_OPT_COUNT_STRETCH: the forms k_row_count_w is built in.
static bool stretch_ok(int v) { return v == -1 || v == 1 || v == 2 || v == 4 || v == 8; }

extern "C" int himg_hip_create(int device, himg_hip_ctx **out) {
  if (!out) return HIMG_ERR_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return HIMG_ERR_HIP;
  if (device < 0 || device >= count) return HIMG_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return HIMG_ERR_HIP;
  himg_hip_ctx *ctx = new himg_hip_ctx();
  ctx->device = device;
  HostOpts &o = ctx->opts;
  if (const char *e = std::getenv("HIMG_FORCE_UNFUSED")) o.allow_fused = !(e[0] == '1');
  if (const char *e = std::getenv("HIMG_WALK_SEGS")) o.walk_segs = atoi(e);
  if (const char *e = std::getenv("HIMG_SIDE_STREAM")) o.use_side = !(e[0] == '0');
  if (const char *e = std::getenv("HIMG_PERSIST_ROWS")) o.persist_rows = atoi(e);
  if (const char *e = std::getenv("HIMG_PREFETCH_ROWS")) ctx->prefetch_rows = atoi(e);
  if (const char *e = std::getenv("HIMG_FIX_T2")) ctx->fix_t2 = e[0] == '1';
  if (const char *e = std::getenv("HIMG_FORCE_LRES_SERIAL")) ctx->lres_serial = e[0] == '1';
  if (const char *e = std::getenv("HIMG_MAX_SUB_BITS")) {
    const int v = std::atoi(e);
    if (v >= 128 && v <= 4096 && v % 32 == 0) ctx->max_sub = v;
  }
  if (const char *e = std::getenv("HIMG_COUNT_WAVE")) ctx->count_wave = atoi(e) ? 1 : 0;
  if (const char *e = std::getenv("HIMG_COUNT_STRETCH")) {
    const int v = std::atoi(e);
    if (stretch_ok(v)) ctx->count_stretch = v;
  }
  if (const char *e = std::getenv("HIMG_EMIT_ROWS")) ctx->emit_rows = atoi(e) ? 1 : 0;
  if (const char *e = std::getenv("HIMG_ROW_TOKENS")) ctx->row_tokens = atoi(e) ? 1 : 0;
  if (const char *e = std::getenv("HIMG_FRONT")) ctx->front = atoi(e) ? 1 : 0;
  if (const char *e = std::getenv("HIMG_LEAD_BITS")) {
    const int v = std::atoi(e);
    if (v >= 0 && v <= 4096) ctx->lead_bits = v;
  }
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0) o.n_cu = n_cu;
  if (himg_dev::enc_set_kernel_attrs() != hipSuccess || himg_dev::dec_set_kernel_attrs() != hipSuccess) {
    delete ctx;
    return HIMG_ERR_HIP;
  }
  // Companding LUT for every magnitude an int16 can take.
  std::vector<uint8_t> lut(32769);
  int16_t fmap[128];
  himg_tables_fullres_map(fmap);
  for (int a = 0; a <= 32767; ++a) lut[a] = himg_tables_map_to_8bit(fmap, a);
  lut[32768] = (uint8_t)(0u - himg_tables_map_to_8bit(fmap, -32768));  // |x| of -32768 (unreachable)
  if (!ctx->fmap_lut.reserve(round_up(lut.size(), 256)) ||
      hipMemcpy(ctx->fmap_lut.p, lut.data(), lut.size(), hipMemcpyHostToDevice) != hipSuccess) {
    delete ctx;
    return HIMG_ERR_HIP;
  }
  // The side stream carries the wide k_row_count next to the caller's stream's short
  // LRES kernels: lowest priority, so that those are placed first whenever a slot
  // frees up (they sit on the critical path of the frame, the counts do not).
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  bool ev_ok = true;
  for (int k = 0; k < kWalkSegs; ++k)
    ev_ok = ev_ok && hipEventCreateWithFlags(&ctx->dstr.ev_walk[k], hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ctx->dstr.ev_cnt[k], hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ctx->dstr.ev_win[k], hipEventDisableTiming) == hipSuccess;
  if (!ev_ok || hipStreamCreateWithPriority(&ctx->dstr.side, hipStreamNonBlocking, prio_least) != hipSuccess ||
      hipStreamCreateWithPriority(&ctx->dstr.side2, hipStreamNonBlocking, prio_least) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->dstr.ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->side_enc, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_fork_e, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_join_e, hipEventDisableTiming) != hipSuccess) {
    himg_hip_destroy(ctx);
    return HIMG_ERR_HIP;
  }
  // The decoder's third helper stream IS the encoder's side stream (a context never encodes and
  // decodes at once): the runtime maps streams onto FOUR hardware queues (GPU_MAX_HW_QUEUES), and
  // a fifth stream of this context shared a queue with another one -- the encoder's LRES branch
  // then ran behind the pixel stage instead of beside it (+1.5 ms per 128-frame step, measured).
  ctx->dstr.side3 = ctx->side_enc;
  *out = ctx;
  return HIMG_OK;
}

static void opened_free(himg_hip_opened *o);

extern "C" void himg_hip_destroy(himg_hip_ctx *ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipDeviceSynchronize();
  for (himg_hip_opened *o : ctx->opened) opened_free(o);
  ctx->opened.clear();
  if (ctx->dstr.ev_fork) hipEventDestroy(ctx->dstr.ev_fork);
  for (int k = 0; k < kWalkSegs; ++k) {
    if (ctx->dstr.ev_walk[k]) hipEventDestroy(ctx->dstr.ev_walk[k]);
    if (ctx->dstr.ev_cnt[k]) hipEventDestroy(ctx->dstr.ev_cnt[k]);
    if (ctx->dstr.ev_win[k]) hipEventDestroy(ctx->dstr.ev_win[k]);
  }
  for (int k = 0; k < HIMG_MAX_WALK_RANGES; ++k)
    if (ctx->ev_range[k]) hipEventDestroy(ctx->ev_range[k]);
  if (ctx->dstr.side) hipStreamDestroy(ctx->dstr.side);
  if (ctx->dstr.side2) hipStreamDestroy(ctx->dstr.side2);
  if (ctx->ev_fork_e) hipEventDestroy(ctx->ev_fork_e);
  if (ctx->ev_join_e) hipEventDestroy(ctx->ev_join_e);
  if (ctx->side_enc) hipStreamDestroy(ctx->side_enc);
  for (int k = 0; k < himg_hip_ctx::SizeRing::kSlots; ++k) {
    if (ctx->sizes_ring.ev[k]) hipEventDestroy(ctx->sizes_ring.ev[k]);
    if (ctx->sizes_ring.h[k]) hipHostFree(ctx->sizes_ring.h[k]);
  }
  ctx->prof.collect();
  if (ctx->pipe.ready) {
    for (int k = 0; k < 2; ++k) {
      hipEventDestroy(ctx->pipe.ev_in[k]); hipEventDestroy(ctx->pipe.ev_k[k]); hipEventDestroy(ctx->pipe.ev_out[k]);
      ctx->pipe.in[k].release(); ctx->pipe.out[k].release(); ctx->pipe.meta[k].release();
    }
    hipStreamDestroy(ctx->pipe.s_in); hipStreamDestroy(ctx->pipe.s_comp); hipStreamDestroy(ctx->pipe.s_out);
    hipHostFree(ctx->pipe.h_meta);
  }
  DevBuf *all[] = {&ctx->fmap_lut, &ctx->e_planes, &ctx->e_lres, &ctx->e_fres, &ctx->e_small,
                   &ctx->e_spanhist, &ctx->e_tok, &ctx->e_tokx, &ctx->e_dbgtree, &ctx->e_qtab, &ctx->e_search, &ctx->e_stab, &ctx->e_rec, &ctx->d_frames, &ctx->d_nodes, &ctx->d_grp, &ctx->d_gyc, &ctx->d_sub, &ctx->d_lane, &ctx->d_rows,
                   &ctx->d_lres, &ctx->d_fres, &ctx->d_planes, &ctx->d_sizes, &ctx->d_stats, &ctx->d_spec, &ctx->d_cmap, &ctx->h_in,
                   &ctx->h_out, &ctx->h_result, &ctx->h_status, &ctx->h_index};
  for (DevBuf *b : all) b->release();
  if (ctx->hp_index) hipHostFree(ctx->hp_index);
  delete ctx;
}

extern "C" const char *himg_hip_last_error(const himg_hip_ctx *ctx) {
  return ctx ? ctx->err.c_str() : "no context";
}

extern "C" void himg_hip_free(void *p) { std::free(p); }

extern "C" void *himg_hip_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
extern "C" void himg_hip_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

extern "C" int himg_hip_get_option(himg_hip_ctx *ctx, int option, int *value) {
  if (!ctx || !value) return HIMG_ERR_ARG;
  if (option == HIMG_OPT_FIX_T2) { *value = ctx->fix_t2; return HIMG_OK; }
  if (option == HIMG_OPT_COUNT_WAVE) { *value = ctx->count_wave; return HIMG_OK; }
  if (option == HIMG_OPT_EMIT_ROWS) { *value = ctx->emit_rows; return HIMG_OK; }
  if (option == HIMG_OPT_ROW_TOKENS) { *value = ctx->row_tokens; return HIMG_OK; }
  if (option == HIMG_OPT_FRONT) { *value = ctx->front; return HIMG_OK; }
  if (option == HIMG_OPT_COUNT_STRETCH) { *value = ctx->count_stretch; return HIMG_OK; }
  return fail(ctx, HIMG_ERR_ARG, "unknown option");
}

extern "C" int himg_hip_set_option(himg_hip_ctx *ctx, int option, int value) {
  if (!ctx) return HIMG_ERR_ARG;
  if (option == HIMG_OPT_FIX_T2) { ctx->fix_t2 = value ? 1 : 0; return HIMG_OK; }
  if (option == HIMG_OPT_COUNT_STRETCH) {
    if (!stretch_ok(value)) return fail(ctx, HIMG_ERR_ARG, "count_stretch: -1, 1, 2, 4 or 8");
    ctx->count_stretch = value;
    return HIMG_OK;
  }
  const int tri = value < 0 ? -1 : (value ? 1 : 0);
  if (option == HIMG_OPT_COUNT_WAVE) { ctx->count_wave = tri; return HIMG_OK; }
  if (option == HIMG_OPT_EMIT_ROWS) { ctx->emit_rows = tri; return HIMG_OK; }
  if (option == HIMG_OPT_FRONT) { ctx->front = tri; return HIMG_OK; }
  if (option == HIMG_OPT_ROW_TOKENS) { ctx->row_tokens = value == 2 ? 2 : tri; return HIMG_OK; }   // (2: on + k_emit_tok's spelled-out path, a test knob)
  return fail(ctx, HIMG_ERR_ARG, "unknown option");
}

// ---------------------------------------------------------------------------
// Host-built tables and container bytes.
// ---------------------------------------------------------------------------
static void put_u32(uint8_t *p, uint32_t x) {
  p[0] = (uint8_t)x; p[1] = (uint8_t)(x >> 8); p[2] = (uint8_t)(x >> 16); p[3] = (uint8_t)(x >> 24);
}

static int build_static(const Geom &g, int quality, StaticChunks *sc, ShiftTables *st,
                        LresTables *lt) {
  memset(sc, 0, sizeof(*sc));
  uint8_t *h = sc->head;
  // encoder.cpp:111-129,139-166
  memcpy(h, "RIFF", 4); put_u32(h + 4, 0); memcpy(h + 8, "HIMG", 4);
  memcpy(h + 12, "FRMT", 4); put_u32(h + 16, 11);
  h[20] = 1; put_u32(h + 21, (uint32_t)g.W); put_u32(h + 25, (uint32_t)g.H);
  h[29] = (uint8_t)g.C; h[30] = (uint8_t)g.ycbcr;
  // encoder.cpp:88-89,168-184
  int16_t lmap[128], fmap[128];
  himg_tables_lowres_map(quality, lmap);
  memcpy(h + 31, "LMAP", 4);
  const int ln = himg_tables_mapping_function(lmap, h + 39);
  if (ln != 128) return HIMG_ERR_UNSUPPORTED;  // low-res tables never exceed 255
  put_u32(h + 35, (uint32_t)ln);
  memcpy(h + 167, "LRES", 4);  // size patched on the device
  // encoder.cpp:95-100,222-256
  himg_tables_shift(quality, 0, st->s[0]);
  himg_tables_shift(quality, 1, st->s[1]);
  uint8_t *m = sc->mid;
  int o = 0;
  memcpy(m + o, "QCFG", 4); put_u32(m + o + 4, g.ycbcr ? 64u : 32u); o += 8;
  for (int t = 0; t < (g.ycbcr ? 2 : 1); ++t)
    for (int i = 0; i < 32; ++i) m[o++] = (uint8_t)((st->s[t][2 * i] << 4) | st->s[t][2 * i + 1]);
  himg_tables_fullres_map(fmap);
  memcpy(m + o, "FMAP", 4);
  const int fn = himg_tables_mapping_function(fmap, m + o + 8);
  put_u32(m + o + 4, (uint32_t)fn);
  o += 8 + fn;
  memcpy(m + o, "FRES", 4); o += 8;  // size patched on the device
  sc->mid_len = o;
  // Low-res companding LUT over every possible prediction error.
  memcpy(lt->tab, lmap, sizeof(lmap));
  for (int d = -255; d <= 255; ++d) lt->code[d + 255] = himg_tables_map_to_8bit(lmap, d);
  lt->code[511] = 0;
  return HIMG_OK;
}

extern "C" int himg_hip_tok_layout(int width, int height, int pixel_stride, int num_channels, int row_tokens,
                                   int batch, int out[6]) {
  Geom g;
  if (!out || batch < 1 || !make_geom(width, height, pixel_stride, num_channels, 1, &g)) return HIMG_ERR_ARG;
  g.row_tokens = row_tokens;
  const int seg = himg_dev::enc_tok_seg(g);
  out[0] = seg;
  out[1] = (g.row_block + seg - 1) / seg;
  out[2] = seg + himg_dev::tok_seg_pad(g.row_block);
  out[3] = himg_dev::tok_stage_need(g.row_block, seg);
  out[4] = himg_dev::kTokStage;
  out[5] = himg_dev::enc_uses_row_tokens(g, batch) ? 1 : 0;
  return HIMG_OK;
}

// ---------------------------------------------------------------------------
// Workspaces.
// ---------------------------------------------------------------------------
// Copy the na words at a, then the nb words at b, into the next pinned slot and start the H2D copy
// from there to d_dst.
static int stage_words(himg_hip_ctx *ctx, void *d_dst, const void *a, size_t na, const void *b, size_t nb, hipStream_t s) {
  auto &r = ctx->sizes_ring;
  const int k = r.next;
  r.next = (k + 1) % himg_hip_ctx::SizeRing::kSlots;
  if (!r.ev[k]) HIP_TRY(ctx, hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming));
  if (r.busy[k]) HIP_TRY(ctx, hipEventSynchronize(r.ev[k]));
  const size_t words = na + nb;
  if (r.cap[k] < words) {
    if (r.h[k]) hipHostFree(r.h[k]);
    r.h[k] = nullptr;
    r.cap[k] = 0;
    const size_t want = words < 64 ? 64 : words;
    HIP_TRY(ctx, hipHostMalloc((void **)&r.h[k], want * 4, hipHostMallocDefault));
    r.cap[k] = want;
  }
  memcpy(r.h[k], a, na * 4);
  if (nb) memcpy(r.h[k] + na, b, nb * 4);
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, r.h[k], words * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipEventRecord(r.ev[k], s));
  r.busy[k] = true;
  return HIMG_OK;
}
// `n` packed sizes on their way to the decoder's d_sizes.  org (the region decode, the decodes into
// pitched pictures): n origins (x, y) follow the sizes, in the same slot and the same copy -- org_sets
// of them, one after the other (the region decode into pictures: the windows', then the destinations').
static int stage_sizes(himg_hip_ctx *ctx, const uint32_t *src, int n, hipStream_t s, const int32_t *org = nullptr,
                       int org_sets = 1) {
  return stage_words(ctx, ctx->d_sizes.p, src, (size_t)n, org, org ? (size_t)n * 2 * (size_t)org_sets : 0, s);
}

static int ensure_enc_ws(himg_hip_ctx *ctx, const Geom &g, int batch, bool allow_row_tokens = true, bool force_row_tokens = false) {
  EncWs &w = ctx->enc_ws;
  // A row-sharded encode in progress belongs to the geometry it was started with.
  {
    const Geom &o = ctx->shard.g;
    if (ctx->shard.valid && (batch != 1 || o.W != g.W || o.H != g.H || o.C != g.C || o.stride != g.stride ||
                             o.ycbcr != g.ycbcr))
      ctx->shard.valid = false;
  }
  const size_t plane = round_up((size_t)g.C * g.rows * g.cols, 256);
  const size_t lres = round_up((size_t)g.lres_size + 16, 256);
  const size_t fres = round_up((size_t)g.fres_size + 16, 256);
  const int nsp = g.lres_spans + g.rows;
  // FRES rows as a token stream between the tokeniser and the bit packer (batches): 16-bit slots,
  // worst case 2 bytes per symbol (+ padding per segment), ~0.7 in use.
  const bool row_tok = allow_row_tokens && (force_row_tokens ? himg_dev::enc_tok_stage_fits(g) : himg_dev::enc_uses_row_tokens(g, batch));
  const int tok_seg = row_tok ? himg_dev::enc_tok_seg(g) : 0;
  const int tok_nseg = row_tok ? (g.row_block + tok_seg - 1) / tok_seg : 0;
  const int tok_cap = tok_seg + himg_dev::tok_seg_pad(g.row_block);   // (no content needs more: himg_dev.h)
  if (!ctx->e_planes.reserve(2 * plane * batch) || !ctx->e_lres.reserve(lres * batch) ||
      !ctx->e_fres.reserve(fres * batch) ||
      (row_tok && !ctx->e_tok.reserve((size_t)batch * g.rows * tok_nseg * ((size_t)tok_cap * 2 + 4))))
    return fail(ctx, HIMG_ERR_HIP, "encoder workspace allocation failed");
  // Small per-frame arrays, carved from one allocation.
  size_t off = 0;
  auto carve = [&](size_t bytes) { size_t o = off; off += round_up(bytes, 256); return o; };
  const size_t o_hist = carve((size_t)batch * 2 * kHistStride * 4);
  const size_t o_codes = carve((size_t)batch * 2 * kHistStride * 8);
  const size_t o_lens = carve((size_t)batch * 2 * kHistStride * 4);
  const size_t o_tree = carve((size_t)batch * 2 * kTreeStride);
  const size_t o_tnb = carve((size_t)batch * 2 * 4);
  const size_t o_trail = carve((size_t)batch * g.lres_spans * 4);
  const size_t o_bit0 = carve((size_t)batch * nsp * 8);
  const size_t o_bits = carve((size_t)batch * nsp * 4);
  const size_t o_status = carve((size_t)batch * 4);
  if (!ctx->e_small.reserve(off) ||
      !ctx->e_spanhist.reserve((size_t)batch * nsp * kHistStride * 4))
    return fail(ctx, HIMG_ERR_HIP, "encoder workspace allocation failed");
  uint8_t *sm = (uint8_t *)ctx->e_small.p;
  w.avg = (uint8_t *)ctx->e_planes.p;
  w.low = w.avg + plane * batch;
  w.plane_stride = plane;
  w.lres_sym = (uint8_t *)ctx->e_lres.p; w.lres_stride = lres;
  w.fres_sym = (uint8_t *)ctx->e_fres.p; w.fres_stride = fres;
  w.tok = row_tok ? (uint16_t *)ctx->e_tok.p : nullptr;
  w.tok_cnt = row_tok ? (uint32_t *)((uint8_t *)ctx->e_tok.p + (size_t)batch * g.rows * tok_nseg * (size_t)tok_cap * 2) : nullptr;
  w.tok_seg = tok_seg; w.tok_nseg = tok_nseg; w.tok_cap = tok_cap;
  w.hist = (uint32_t *)(sm + o_hist);
  w.codes = (uint64_t *)(sm + o_codes);
  w.lens = (uint32_t *)(sm + o_lens);
  w.tree = sm + o_tree;
  w.tree_nbytes = (uint32_t *)(sm + o_tnb);
  w.lres_trail = (uint32_t *)(sm + o_trail);
  w.span_bit0 = (uint64_t *)(sm + o_bit0);
  w.span_bits = (uint32_t *)(sm + o_bits);
  w.status = (int32_t *)(sm + o_status);
  w.span_hist_l = (uint32_t *)ctx->e_spanhist.p;
  w.span_hist_f = w.span_hist_l + (size_t)batch * g.lres_spans * kHistStride;
  ctx->enc_geom = g;
  ctx->enc_batch = batch;
  ctx->enc_valid = true;
  return HIMG_OK;
}

// Rows wider than the LDS: does a quarter sub-sequence (1 / 4096 of a row's payload) of the
// LARGEST stream of the call fit k_row_count_q's staging buffer, with a margin for rows above
// the frame's mean?  (An estimate from the stream's size; a row that exceeds it anyway is left
// to k_dec_huff by the kernel itself.)
static int wide_q_hint(const Geom &g, uint32_t max_packed_size) {
  if (himg_dev::dec_rows_fit_lds(g) || g.rows < 1) return 0;
  const double bits_per_quarter = 8.0 * (double)max_packed_size / ((double)g.rows * 4096.0);
  return bits_per_quarter <= 272.0 ? 1 : 0;   // kStageSubBits = 320: rows up to 17 % above the mean
}

// head_only (the 1/8-scale preview): what the head phase touches and nothing of the FRES rows --
// no row index, lane records or FRES symbol plane (a 16384^2 frame's would be hundreds of MB),
// the LRES stream's tables only; d_sizes holds the packed sizes, then where each LRES chunk ends.
// region (the region decode): no FRES symbol plane and no quarter records either; d_sizes holds the
// packed sizes, then each frame's origin (x, y).  (Either kind has room for two origins per frame
// behind the sizes: a destination origin, decode_full / region_launch.)
enum DecWsKind { kWsFull, kWsHead, kWsRegion };
static int ensure_dec_ws(himg_hip_ctx *ctx, const Geom &g, int batch, DecWsKind kind) {
  const bool head_only = kind == kWsHead, region = kind == kWsRegion;
  DecWs &w = ctx->dec_ws;
  ctx->head.valid = false;   // whatever decode this is, it overwrites what a head phase left
  const size_t plane = round_up((size_t)g.C * g.rows * g.cols, 256);
  const size_t lres = round_up((size_t)g.lres_size + 16, 256);
  const size_t fres = round_up((size_t)g.fres_size + 16, 256);
  if (head_only) {
    // The tables keep their [frame][stream] layout: frame f's LRES tables at 2 f, the last one at 2 batch - 2.
    const size_t nst = 2 * (size_t)batch - 1;
    if (!ctx->d_frames.reserve(sizeof(DecFrame) * batch) || !ctx->d_nodes.reserve(nst * (2 * kNumSym) * 4) ||
        !ctx->d_grp.reserve(nst * (1u << kLutBits) * 8) || !ctx->d_gyc.reserve(nst * (1u << kLutBits) * 4) ||
        !ctx->d_sub.reserve(nst * kSubEntries * 8) || !ctx->d_lres.reserve(lres * batch) ||
        !ctx->d_planes.reserve(plane * batch) || !ctx->d_sizes.reserve((size_t)batch * 8) ||
        !ctx->d_stats.reserve(((size_t)batch * (g.rows + 1) * 8 + (size_t)batch * 4) * 4))
      return fail(ctx, HIMG_ERR_HIP, "decoder workspace allocation failed");
  } else if (!ctx->d_frames.reserve(sizeof(DecFrame) * batch) ||
      !ctx->d_nodes.reserve((size_t)batch * 2 * (2 * kNumSym) * 4) ||
      !ctx->d_grp.reserve((size_t)batch * 2 * (1u << kLutBits) * 8) ||
      !ctx->d_gyc.reserve((size_t)batch * 2 * (1u << kLutBits) * 4) ||
      !ctx->d_sub.reserve((size_t)batch * 2 * kSubEntries * 8) ||
      !ctx->d_lane.reserve((size_t)batch * g.rows * (2 * kDecThreads + himg_dev::kRecHdr + (region || himg_dev::dec_rows_fit_lds(g) ? 0 : 6 * kDecThreads)) * 4) ||
      !ctx->d_rows.reserve((size_t)batch * g.rows * 4 * 2) || !ctx->d_lres.reserve(lres * batch) ||
      (!region && !ctx->d_fres.reserve(fres * batch)) || !ctx->d_planes.reserve(plane * batch) ||
      !ctx->d_sizes.reserve((size_t)batch * 32) ||   // (launch_prefix's eight words per frame are the most)
      !ctx->d_stats.reserve(((size_t)batch * (g.rows + 1) * 8 + (size_t)batch * 4 + (size_t)batch * g.rows * 8) * 4))
    return fail(ctx, HIMG_ERR_HIP, "decoder workspace allocation failed");
  w.frames = (DecFrame *)ctx->d_frames.p;
  w.nodes = (uint32_t *)ctx->d_nodes.p;
  w.grp = (uint2 *)ctx->d_grp.p;
  w.gyc = (uint32_t *)ctx->d_gyc.p;
  w.sub = (uint2 *)ctx->d_sub.p;
  w.lane_start = head_only ? nullptr : (uint32_t *)ctx->d_lane.p;
  w.lane_off = head_only ? nullptr : w.lane_start + (size_t)batch * g.rows * kDecThreads;
  w.lane_q = (head_only || region || himg_dev::dec_rows_fit_lds(g)) ? nullptr : w.lane_off + (size_t)batch * g.rows * (kDecThreads + himg_dev::kRecHdr);
  w.row_off = head_only ? nullptr : (uint32_t *)ctx->d_rows.p;
  w.row_len = head_only ? nullptr : w.row_off + (size_t)batch * g.rows;
  w.lres_sym = (uint8_t *)ctx->d_lres.p; w.lres_stride = lres;
  w.fres_sym = (head_only || region) ? nullptr : (uint8_t *)ctx->d_fres.p; w.fres_stride = (head_only || region) ? 0 : fres;
  w.low = (uint8_t *)ctx->d_planes.p; w.plane_stride = plane;
  w.stats = (uint32_t *)ctx->d_stats.p;
  w.parse_stats = w.stats + (size_t)batch * (g.rows + 1) * 8;
  w.rc_stats = head_only ? nullptr : w.parse_stats + (size_t)batch * 4;
  {
    // LRES payload <= lres_size + tree bytes (huffman_enc.cpp:242-244).
    const size_t max_bits = 8ull * ((size_t)g.lres_size + kTreeStride);
    const size_t cb = (size_t)kDecThreads * kLresSubBits;   // bits per chunk (kLresChunkBits of kernels_dec.hip)
    int nch = (int)((max_bits + cb - 1) / cb);
    if (nch > 1024) nch = 1024;  // beyond this the serial path takes over (k_lres_fix)
    w.lres_chunks = nch;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += round_up(bytes, 256); return o; };
    const size_t o_ss = carve((size_t)batch * nch * kDecThreads * 4);
    const size_t o_sc = carve((size_t)batch * nch * kDecThreads * 4);
    const size_t o_se = carve((size_t)batch * nch * 8);
    const size_t o_st = carve((size_t)batch * nch * 8);
    const size_t o_sp = carve((size_t)batch * nch * kDecThreads * 4);
    const size_t o_fe = carve((size_t)batch * nch * 8);
    const size_t o_vb = carve((size_t)batch * nch * 8);
    const size_t o_ok = carve((size_t)batch * 4);
    const size_t o_eb = carve((size_t)batch * 8);
    const size_t o_mm = carve((size_t)batch * nch * kDecThreads * 4 * himg_dev::kLresMemoWords);
    if (!ctx->d_spec.reserve(off)) return fail(ctx, HIMG_ERR_HIP, "decoder workspace allocation failed");
    uint8_t *b = (uint8_t *)ctx->d_spec.p;
    w.spec_start = (uint32_t *)(b + o_ss); w.spec_cnt = (uint32_t *)(b + o_sc);
    w.spec_end = (uint64_t *)(b + o_se); w.spec_tot = (uint64_t *)(b + o_st);
    w.spec_endpos = (uint32_t *)(b + o_sp); w.fix_end = (uint64_t *)(b + o_fe);
    w.ver_base = (uint64_t *)(b + o_vb); w.ver_ok = (int32_t *)(b + o_ok);
    w.lres_endbit = (uint64_t *)(b + o_eb);
    w.spec_memo = (uint32_t *)(b + o_mm);
  }
  ctx->dec_geom = g;
  ctx->dec_batch = batch;
  ctx->dec_valid = true;
  return HIMG_OK;
}

// Text the reference prints for a failed stage (decoder.cpp:96-135,232,287,345).
static std::string format_message(int32_t st) {
  static const char *kStage[] = {"", "Not a RIFF HIMG file.\n", "Error decoding header.\n",
                                 "Error decoding low-res mapping function.\n",
                                 "Error decoding low-res data.\n",
                                 "Error decoding quantization configuration.\n",
                                 "Error decoding full-res mapping function.\n",
                                 "Error decoding full-res data.\n"};
  std::string m;
  if (st & 0x100) m += "Error: Invalid Huffman data.\n";
  const int stage = (st >> 4) & 7;
  m += kStage[stage];
  return m;
}

static int status_to_code(int32_t st) {
  st &= 15;
  switch (st) {
    case 0: return HIMG_OK;
    case 1: return HIMG_ERR_ARG;
    case 3: return HIMG_ERR_UNSUPPORTED;
    case 4: return HIMG_ERR_FORMAT;
    case 5: return HIMG_ERR_CAPACITY;
    default: return HIMG_ERR_HIP;
  }
}

// A device status as the host API reports it: the reference's message for a format error, else `what`.
static const char kDecodeError[] = "device decode reported an error";
static int status_error(himg_hip_ctx *ctx, int32_t st, const char *what = kDecodeError) {
  const int code = status_to_code(st);
  if (code == HIMG_ERR_FORMAT) ctx->err = format_message(st);
  else fail(ctx, code, what);
  return code;
}

// ---------------------------------------------------------------------------
// Device-resident API.
// ---------------------------------------------------------------------------
// The preamble of every decode entry point, in two steps: the checks, which touch nothing, then the
// reservation.  (Two, because decode_device and decode_walk_ranges_device have a check of their own
// between them: nothing is reserved before every check has passed.)
//
// The checks: the geometry with the context's settings, the grid limit (kWsHead: the preview's, whose
// grids are the low-res plane's) and the alignment rule -- in_stride given: a batch at that stride,
// else one stream.  bad: what the call site found wrong with its own arguments (a row range, a
// rectangle), reported behind a bad geometry.
static int decode_args(himg_hip_ctx *ctx, int width, int height, int num_channels, int batch, DecWsKind kind,
                       const void *d_packed, const void *d_out, const size_t *in_stride, const char *bad, Geom *g) {
  if (!make_geom(width, height, num_channels, num_channels, 1, g)) return fail(ctx, HIMG_ERR_ARG, "bad geometry");
  apply_settings(ctx, g);
  if (bad) return fail(ctx, HIMG_ERR_ARG, bad);
  if ((kind == kWsHead ? g->mrows : g->rows + 1) > 65535 || batch * g->C > 65535)
    return fail(ctx, HIMG_ERR_UNSUPPORTED, "grid too large");
  if ((in_stride && (*in_stride & 3)) || ((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 15))
    return fail(ctx, HIMG_ERR_ARG, in_stride ? "in_stride must be a multiple of 4; buffers 16-byte aligned"
                                             : "buffers must be 16-byte aligned");
  return HIMG_OK;
}

// The reservation: the device, the workspace, the caller's stream as the context's last one, and the
// packed sizes (org: with each frame's origins, see stage_sizes) on their way to *d_sizes.
static int decode_begin(himg_hip_ctx *ctx, const Geom &g, int batch, DecWsKind kind, const uint32_t *h_sizes,
                        void *stream, const uint32_t **d_sizes, const int32_t *org = nullptr, int org_sets = 1) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure_dec_ws(ctx, g, batch, kind)) return rc;
  ctx->last_stream = (hipStream_t)stream;
  if (int rc = stage_sizes(ctx, h_sizes, batch, ctx->last_stream, org, org_sets)) return rc;
  *d_sizes = (const uint32_t *)ctx->d_sizes.p;
  return HIMG_OK;
}

static int stride_covers(himg_hip_ctx *ctx, const uint32_t *h_sizes, int batch, size_t in_stride) {
  for (int i = 0; i < batch; ++i)
    if (((size_t)h_sizes[i] + 3) / 4 * 4 > in_stride)
      return fail(ctx, HIMG_ERR_ARG, "in_stride must cover every stream rounded up to 4 bytes");
  return HIMG_OK;
}

static const char *bad_row_range(int height, int row0, int row1) {
  return row0 < 0 || row1 < row0 || row1 > ((height + 7) >> 3) ? "bad row range" : nullptr;
}

__global__ void k_copy_status(const int32_t *src, int32_t *dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// ---- the encode entry points -----------------------------------------------------------------

struct Enc {
  Geom g;
  hipStream_t s;
  // The per-quality forms (enc_q_begin):
  StaticChunks sc;   // (the container's quality-independent bytes; LMAP / QCFG come from the table)
  QualSel qs;
  SearchState ss;    // the per-frame words of the launch in e_search; the plain per-quality forms use its qualities alone
  himg_dev::SseArgs sa;
};
// What every encode entry point begins with: the checks (need_out: with the output buffer's), the
// workspace, the caller's stream as the context's last one.
static int enc_begin(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height, int pixel_stride,
                     int num_channels, int use_ycbcr, bool need_out, const void *d_out, size_t out_stride,
                     void *stream, Enc *e) {
  if (!d_frames || (need_out && !d_out) || batch < 1 || batch > 65535) return fail(ctx, HIMG_ERR_ARG, "bad argument");
  if (!make_geom(width, height, pixel_stride, num_channels, use_ycbcr, &e->g))
    return fail(ctx, HIMG_ERR_ARG, "bad geometry");
  apply_settings(ctx, &e->g);
  if (e->g.rows > 65535 || batch * e->g.C > 65535) return fail(ctx, HIMG_ERR_UNSUPPORTED, "grid too large");
  if (need_out && ((out_stride & 255) || out_stride < 1024 || ((uintptr_t)d_out & 15)))
    return fail(ctx, HIMG_ERR_ARG, "out_stride must be a multiple of 256; buffers 16-byte aligned");
  if ((uintptr_t)d_frames & 15)
    return fail(ctx, HIMG_ERR_ARG, need_out ? "out_stride must be a multiple of 256; buffers 16-byte aligned"
                                            : "buffers must be 16-byte aligned");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure_enc_ws(ctx, e->g, batch)) return rc;
  e->s = (hipStream_t)stream;
  ctx->last_stream = e->s;
  return HIMG_OK;
}
// ... and ends with: the workspace's status words to d_status (the searches' finish kernel has written
// them: nullptr), and whatever a launch has reported.
static int enc_end(himg_hip_ctx *ctx, const Enc &e, int batch, int32_t *d_status) {
  if (d_status)
    hipLaunchKernelGGL(k_copy_status, dim3((batch + 63) / 64), dim3(64), 0, e.s, ctx->enc_ws.status, d_status, batch);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_encode_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width,
                                      int height, int pixel_stride, int num_channels, int quality,
                                      int use_ycbcr, void *d_out, size_t out_stride,
                                      uint32_t *d_sizes, int32_t *d_status, void *stream) {
  if (!ctx || !d_sizes) return HIMG_ERR_ARG;
  Enc e;
  int rc = enc_begin(ctx, d_frames, batch, width, height, pixel_stride, num_channels, use_ycbcr, true, d_out, out_stride,
                     stream, &e);
  if (rc) return rc;
  StaticChunks sc;
  ShiftTables st;
  LresTables lt;
  rc = build_static(e.g, quality, &sc, &st, &lt);
  if (rc) return fail(ctx, rc, "unsupported table configuration");
  launch_encode(e.g, ctx->enc_ws, batch, (const uint8_t *)d_frames, (uint8_t *)d_out, out_stride,
                d_sizes, sc, st, lt, (const uint8_t *)ctx->fmap_lut.p, e.s, &ctx->prof,
                ctx->opts.use_side ? ctx->side_enc : nullptr, ctx->ev_fork_e, ctx->ev_join_e);
  return enc_end(ctx, e, batch, d_status);
}

// ---- quality per frame, size-only pass, distortion probe, the searches ------------------------

// The tables of every quality, in HBM: built on the context's first such call (the one place where
// these calls wait for the device).
static int ensure_qual_tab(himg_hip_ctx *ctx) {
  if (ctx->qtab_ready) return HIMG_OK;
  Geom g;
  if (!make_geom(8, 8, 4, 4, 1, &g)) return fail(ctx, HIMG_ERR_ARG, "bad geometry");   // (any geometry with a chroma table)
  std::vector<QualTab> tabs(kQualities);
  std::vector<himg_dev::SseTab> stabs(kQualities);
  // The magnitudes a decoder reads back from the FMAP chunk (serialised and parsed, as a stream carries them).
  int16_t fmap[128], fmap_dec[128];
  uint8_t fbuf[512];
  himg_tables_fullres_map(fmap);
  const int fn = himg_tables_mapping_function(fmap, fbuf);
  if (fn <= 0 || fn > (int)sizeof(fbuf) || himg_tables_parse_mapping_function(fmap_dec, fbuf, fn) != 1)
    return fail(ctx, HIMG_ERR_UNSUPPORTED, "unsupported table configuration");
  for (int q = 0; q < kQualities; ++q) {
    StaticChunks sc;
    ShiftTables st;
    LresTables lt;
    const int rc = build_static(g, q, &sc, &st, &lt);
    if (rc) return fail(ctx, rc, "unsupported table configuration");
    himg_dev::enc_fill_qual_tab(sc, st, lt, &tabs[q]);
    himg_dev::sse_fill_tab(fmap_dec, st, &stabs[q]);
  }
  if (!ctx->e_qtab.reserve(round_up(tabs.size() * sizeof(QualTab), 256)) ||
      !ctx->e_stab.reserve(round_up(stabs.size() * sizeof(himg_dev::SseTab), 256)))
    return fail(ctx, HIMG_ERR_HIP, "quality table allocation failed");
  HIP_TRY(ctx, hipMemcpy(ctx->e_qtab.p, tabs.data(), tabs.size() * sizeof(QualTab), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->e_stab.p, stabs.data(), stabs.size() * sizeof(himg_dev::SseTab), hipMemcpyHostToDevice));
  ctx->qtab_ready = true;
  return HIMG_OK;
}

// enc_begin for the forms that take their tables by each frame's quality: the table, the per-frame
// words, and (sse: the distortion probe runs) the reconstructed low-res planes beside the workspace's.
static int enc_q_begin(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height, int pixel_stride,
                       int num_channels, int use_ycbcr, bool need_out, const void *d_out, size_t out_stride, bool sse,
                       void *stream, Enc *e) {
  int rc = enc_begin(ctx, d_frames, batch, width, height, pixel_stride, num_channels, use_ycbcr, need_out, d_out,
                     out_stride, stream, e);
  if (rc) return rc;
  if ((rc = ensure_qual_tab(ctx))) return rc;
  if (!ctx->e_search.reserve(round_up(himg_dev::search_state_bytes(batch), 256)) ||
      (sse && !ctx->e_rec.reserve(ctx->enc_ws.plane_stride * (size_t)batch)))
    return fail(ctx, HIMG_ERR_HIP, "encoder workspace allocation failed");
  ShiftTables st;
  LresTables lt;
  rc = build_static(e->g, 50, &e->sc, &st, &lt);
  if (rc) return fail(ctx, rc, "unsupported table configuration");
  e->ss = himg_dev::search_state_carve(ctx->e_search.p, batch);
  e->qs.tab = (const QualTab *)ctx->e_qtab.p;
  e->qs.quality = e->ss.quality;
  e->sa.rec = (uint8_t *)ctx->e_rec.p;
  e->sa.tab = (const himg_dev::SseTab *)ctx->e_stab.p;
  e->sa.sse = nullptr;   // (sse_launch: the caller's, or SearchState::value)
  return HIMG_OK;
}
static void enc_q_launch(himg_hip_ctx *ctx, const Enc &e, int batch, const void *d_frames, void *d_out, size_t out_stride,
                         uint32_t *d_sizes) {
  launch_encode_q(e.g, ctx->enc_ws, batch, (const uint8_t *)d_frames, (uint8_t *)d_out, out_stride, d_sizes, e.sc, e.qs,
                  (const uint8_t *)ctx->fmap_lut.p, e.s, &ctx->prof, ctx->opts.use_side ? ctx->side_enc : nullptr,
                  ctx->ev_fork_e, ctx->ev_join_e);
}
static void sse_launch(himg_hip_ctx *ctx, const Enc &e, int batch, const void *d_frames, uint64_t *d_sse) {
  himg_dev::SseArgs sa = e.sa;
  sa.sse = d_sse;
  himg_dev::launch_encode_sse(e.g, ctx->enc_ws, batch, (const uint8_t *)d_frames, e.sc, e.qs, sa,
                              (const uint8_t *)ctx->fmap_lut.p, e.s, &ctx->prof,
                              ctx->opts.use_side ? ctx->side_enc : nullptr, ctx->ev_fork_e, ctx->ev_join_e);
}
static bool qualities_ok(const int32_t *h_quality, int batch) {
  if (!h_quality) return false;
  for (int i = 0; i < batch; ++i)
    if (h_quality[i] < 0 || h_quality[i] > 100) return false;
  return true;
}

// The three forms with a quality per frame from the host: the streams (need_out), their sizes alone
// (d_sizes without d_out), or their distortions (d_sse, no sizes).
static int encode_q_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height, int pixel_stride,
                           int num_channels, const int32_t *h_quality, int use_ycbcr, bool need_out, void *d_out,
                           size_t out_stride, uint32_t *d_sizes, uint64_t *d_sse, int32_t *d_status, void *stream) {
  if (!ctx) return HIMG_ERR_ARG;
  if (batch < 1 || !qualities_ok(h_quality, batch)) return fail(ctx, HIMG_ERR_ARG, "a quality outside [0, 100]");
  if (d_sse ? ((uintptr_t)d_sse & 7) != 0 : !d_sizes) return fail(ctx, HIMG_ERR_ARG, "bad argument");
  Enc e;
  int rc = enc_q_begin(ctx, d_frames, batch, width, height, pixel_stride, num_channels, use_ycbcr, need_out, d_out,
                       out_stride, d_sse != nullptr, stream, &e);
  if (rc) return rc;
  if ((rc = stage_words(ctx, e.ss.quality, h_quality, (size_t)batch, nullptr, 0, e.s))) return rc;
  if (d_sse) sse_launch(ctx, e, batch, d_frames, d_sse);
  else enc_q_launch(ctx, e, batch, d_frames, d_out, out_stride, d_sizes);
  return enc_end(ctx, e, batch, d_status);
}

extern "C" int himg_hip_encode_device_q(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                        int pixel_stride, int num_channels, const int32_t *h_quality, int use_ycbcr,
                                        void *d_out, size_t out_stride, uint32_t *d_sizes, int32_t *d_status,
                                        void *stream) {
  return encode_q_device(ctx, d_frames, batch, width, height, pixel_stride, num_channels, h_quality, use_ycbcr, true,
                         d_out, out_stride, d_sizes, nullptr, d_status, stream);
}

extern "C" int himg_hip_encode_sizes_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                            int pixel_stride, int num_channels, const int32_t *h_quality,
                                            int use_ycbcr, uint32_t *d_sizes, int32_t *d_status, void *stream) {
  return encode_q_device(ctx, d_frames, batch, width, height, pixel_stride, num_channels, h_quality, use_ycbcr, false,
                         nullptr, 0, d_sizes, nullptr, d_status, stream);
}

extern "C" int himg_hip_encode_sse_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                          int pixel_stride, int num_channels, const int32_t *h_quality, int use_ycbcr,
                                          uint64_t *d_sse, int32_t *d_status, void *stream) {
  return encode_q_device(ctx, d_frames, batch, width, height, pixel_stride, num_channels, h_quality, use_ycbcr, false,
                         nullptr, 0, nullptr, d_sse, d_status, stream);
}

// ---- windows of pitched source pictures -------------------------------------------------------

// The host checks of a source descriptor and its windows (include/himg_hip.h); *bytes: the end of the
// last byte a window owns.  Returns what is wrong, or nullptr.  (dst_check: the same rules for the
// pictures a decode writes into.)
static const char *windows_check(const himg_hip_src *src, int num_channels, int batch, const int32_t *h_origins, int w,
                                 int h, size_t *bytes) {
  if (!src || !h_origins || batch < 1) return "bad argument";
  if (src->width < 1 || src->height < 1 || w < 1 || h < 1) return "a picture or window size that is not positive";
  if (num_channels < 1 || num_channels > 4 || src->pixel_stride < num_channels) return "pixel_stride below num_channels";
  typedef unsigned __int128 u128;
  const u128 ps = (u128)src->pixel_stride, rp = src->row_pitch, fp = src->frame_pitch;
  if (rp < (u128)src->width * ps) return "row_pitch below width * pixel_stride";
  if (fp != 0 && fp < (u128)(src->height - 1) * rp + (u128)src->width * ps) return "frame_pitch neither 0 nor a whole picture";
  if (src->pixel_stride == 4 && ((src->row_pitch | src->frame_pitch) & 3))
    return "row_pitch and frame_pitch must be multiples of 4 for 4-byte pixels";
  u128 end = 0;
  for (int f = 0; f < batch; ++f) {
    const int x = h_origins[2 * f], y = h_origins[2 * f + 1];
    if (x < 0 || y < 0 || w > src->width - x || h > src->height - y) return "a window outside its picture";
    const u128 e = (u128)f * fp + (u128)(y + h - 1) * rp + (u128)(x + w) * ps;
    if (e > end) end = e;
  }
  if (end > (u128)SIZE_MAX) return "pictures that do not fit the address space";
  *bytes = (size_t)end;
  return nullptr;
}

extern "C" int himg_hip_windows_extent(const himg_hip_src *src, int num_channels, int batch, const int32_t *h_origins,
                                       int w, int h, size_t *bytes) {
  if (!bytes) return HIMG_ERR_ARG;
  *bytes = 0;
  return windows_check(src, num_channels, batch, h_origins, w, h, bytes) ? HIMG_ERR_ARG : HIMG_OK;
}

extern "C" int himg_hip_encode_windows_device(himg_hip_ctx *ctx, const void *d_src, const himg_hip_src *src, int batch,
                                              int num_channels, const int32_t *h_origins, int w, int h,
                                              const int32_t *h_quality, int use_ycbcr, void *d_out, size_t out_stride,
                                              uint32_t *d_sizes, int32_t *d_status, void *stream) {
  if (!ctx || !d_sizes) return HIMG_ERR_ARG;
  size_t extent = 0;
  if (const char *bad = windows_check(src, num_channels, batch, h_origins, w, h, &extent)) return fail(ctx, HIMG_ERR_ARG, bad);
  if (!qualities_ok(h_quality, batch)) return fail(ctx, HIMG_ERR_ARG, "a quality outside [0, 100]");
  // The workspace and every kernel behind the four that read pixels belong to the WINDOW's geometry.
  Enc e;
  int rc = enc_q_begin(ctx, d_src, batch, w, h, src->pixel_stride, num_channels, use_ycbcr, true, d_out, out_stride, false,
                       stream, &e);
  if (rc) return rc;
  // The qualities and the origins in one copy: SearchState's first two arrays (a frame's 64-bit limit
  // is the room of its two origin words; no search runs here).
  const size_t org_at = (size_t)((int32_t *)e.ss.limit - e.ss.quality);
  std::vector<int32_t> w0(org_at + 2 * (size_t)batch, 0);
  memcpy(w0.data(), h_quality, (size_t)batch * 4);
  memcpy(w0.data() + org_at, h_origins, (size_t)batch * 8);
  if ((rc = stage_words(ctx, e.ss.quality, w0.data(), w0.size(), nullptr, 0, e.s))) return rc;
  const himg_dev::WinSrc ws = {(const uint8_t *)d_src, src->row_pitch, src->frame_pitch, (const int32_t *)e.ss.limit};
  himg_dev::launch_encode_windows(e.g, ctx->enc_ws, batch, ws, (uint8_t *)d_out, out_stride, d_sizes, e.sc, e.qs,
                                  (const uint8_t *)ctx->fmap_lut.p, e.s, &ctx->prof,
                                  ctx->opts.use_side ? ctx->side_enc : nullptr, ctx->ev_fork_e, ctx->ev_join_e);
  return enc_end(ctx, e, batch, d_status);
}

extern "C" int himg_hip_budget_probes(int qmin, int qmax) {
  if (qmin < 0 || qmax > 100 || qmin > qmax) return HIMG_ERR_ARG;
  if (qmin == qmax) return 1;
  int n = 2;
  for (int d = qmax - qmin; d > 1; d = (d + 1) >> 1) ++n;   // + ceil(log2(qmax - qmin))
  return n;
}

// A search over [qmin, qmax] on the device (himg_hip_encode_budget_device / _target_device).
struct EncSearch {
  int dir;           // kSearchFromMin / kSearchFromMax: the end the first probe is at
  bool probe_sse;    // the probe: sse_launch, its values in SearchState::value; else the size-only enc_q_launch, in d_sizes
  int miss_code;     // the status of a frame whose first probe misses its limit
  uint64_t *d_sse;   // where the value at the chosen quality goes, or nullptr
};
// L: the limits as the ABI has them (32-bit budgets, 64-bit targets); the device takes 64-bit ones.
template <typename L>
static int encode_search_device(himg_hip_ctx *ctx, const EncSearch &k, const void *d_frames, int batch, int width,
                                int height, int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                                const L *h_limits, void *d_out, size_t out_stride, uint32_t *d_sizes, int32_t *d_quality,
                                int32_t *d_status, void *stream) {
  if (!ctx) return HIMG_ERR_ARG;
  const int probes = himg_hip_budget_probes(qmin, qmax);
  if (probes < 0) return fail(ctx, HIMG_ERR_ARG, "the quality range must satisfy 0 <= qmin <= qmax <= 100");
  if (!h_limits || !d_sizes || !d_quality || (k.probe_sse && (!k.d_sse || ((uintptr_t)k.d_sse & 7))))
    return fail(ctx, HIMG_ERR_ARG, "bad argument");
  Enc e;
  int rc = enc_q_begin(ctx, d_frames, batch, width, height, pixel_stride, num_channels, use_ycbcr, true, d_out, out_stride,
                       k.probe_sse, stream, &e);
  if (rc) return rc;
  // The first probe's qualities and the limits, in one copy: SearchState's first two arrays.
  const size_t lim_at = (size_t)((int32_t *)e.ss.limit - e.ss.quality);
  std::vector<int32_t> w0(lim_at + 2 * (size_t)batch, k.dir == himg_dev::kSearchFromMin ? qmin : qmax);
  for (int i = 0; i < batch; ++i) {
    const uint64_t lim = h_limits[i];
    memcpy(w0.data() + lim_at + 2 * (size_t)i, &lim, 8);
  }
  if ((rc = stage_words(ctx, e.ss.quality, w0.data(), w0.size(), nullptr, 0, e.s))) return rc;
  for (int p = 0; p < probes; ++p) {
    // (every probe zeroes its own histograms or sums, and its status words)
    if (k.probe_sse) sse_launch(ctx, e, batch, d_frames, e.ss.value);
    else enc_q_launch(ctx, e, batch, d_frames, nullptr, 0, d_sizes);
    himg_dev::launch_search_step(e.ss, ctx->enc_ws, batch, p, probes, k.dir, qmin, qmax, k.probe_sse ? nullptr : d_sizes,
                                 d_quality, e.s, &ctx->prof);
  }
  enc_q_launch(ctx, e, batch, d_frames, d_out, out_stride, d_sizes);
  himg_dev::launch_search_finish(e.ss, ctx->enc_ws, batch, k.miss_code, d_sizes, k.d_sse, d_status, e.s, &ctx->prof);
  return enc_end(ctx, e, batch, nullptr);
}

extern "C" int himg_hip_encode_budget_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                             int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                                             const uint32_t *h_budgets, void *d_out, size_t out_stride,
                                             uint32_t *d_sizes, int32_t *d_quality, int32_t *d_status, void *stream) {
  const EncSearch k = {himg_dev::kSearchFromMin, false, HIMG_ERR_CAPACITY, nullptr};
  return encode_search_device(ctx, k, d_frames, batch, width, height, pixel_stride, num_channels, qmin, qmax, use_ycbcr,
                              h_budgets, d_out, out_stride, d_sizes, d_quality, d_status, stream);
}

extern "C" int himg_hip_encode_target_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                             int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                                             const uint64_t *h_max_sse, void *d_out, size_t out_stride,
                                             uint32_t *d_sizes, int32_t *d_quality, uint64_t *d_sse, int32_t *d_status,
                                             void *stream) {
  const EncSearch k = {himg_dev::kSearchFromMax, true, HIMG_ERR_TARGET, d_sse};
  return encode_search_device(ctx, k, d_frames, batch, width, height, pixel_stride, num_channels, qmin, qmax, use_ycbcr,
                              h_max_sse, d_out, out_stride, d_sizes, d_quality, d_status, stream);
}

extern "C" int himg_hip_psnr_to_sse(double psnr_db, int width, int height, int num_channels, uint64_t *max_sse) {
  Geom g;
  if (!max_sse || !std::isfinite(psnr_db) || psnr_db < 0.0 ||
      !make_geom(width, height, num_channels, num_channels, 1, &g))
    return HIMG_ERR_ARG;
  const double n = (double)width * (double)height * (double)num_channels;
  *max_sse = (uint64_t)floor(255.0 * 255.0 * n / pow(10.0, psnr_db / 10.0));
  return HIMG_OK;
}

// The launch behind the full decodes of a batch in HBM, in the caller's form: the interleaved bytes
// (himg_hip_decode_device), the planar float output, windows of pitched pictures (with each frame's
// origin in h_org: the origins ride with the sizes, the descriptor's org is filled in here), the
// picture pyramid (d_out its level 0) or the stream's own planes.  bad: what the caller found wrong with its descriptor.
static int decode_full(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_sizes, int batch,
                       int width, int height, int num_channels, void *d_out, int32_t *d_status, void *stream,
                       const char *bad = nullptr, himg_dev::StoreForm form = himg_dev::StoreForm(),
                       const int32_t *h_org = nullptr) {
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, batch, kWsFull, d_packed, d_out, &in_stride, bad, &g))
    return rc;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  { uint32_t mx = 0; for (int i = 0; i < batch; ++i) mx = h_sizes[i] > mx ? h_sizes[i] : mx; g.wide_q = wide_q_hint(g, mx); }
  const bool pitch = form.kind == himg_dev::kStorePitch;
  if (int rc = decode_begin(ctx, g, batch, kWsFull, h_sizes, stream, &d_sizes, pitch ? h_org : nullptr)) return rc;
  himg_dev::DstDesc dd;
  if (pitch) {
    dd = form.dst();
    dd.org = (const int32_t *)(d_sizes + batch);
    form = &dd;
  }
  launch_decode(g, ctx->dec_ws, batch, (const uint8_t *)d_packed, in_stride, d_sizes, (uint8_t *)d_out, d_status,
                (hipStream_t)stream, &ctx->prof, ctx->opts, ctx->opts.use_side ? &ctx->dstr : nullptr, 0, g.rows,
                nullptr, false, 3, form);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                      const uint32_t *h_sizes, int batch, int width, int height,
                                      int num_channels, void *d_out, int32_t *d_status,
                                      void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_out || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  return decode_full(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, d_out, d_status, stream);
}

// The row records alone (include/himg_hip.h): what himg_hip_decode_device launches in front of its row
// kernels, with the wavefront-per-row count kernel whatever the batch size.
extern "C" int himg_hip_debug_row_records(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                          const uint32_t *h_sizes, int batch, int width, int height,
                                          int num_channels, int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_status || batch < 1 || batch > 65535) return HIMG_ERR_ARG;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, batch, kWsFull, d_packed, nullptr, &in_stride, nullptr, &g))
    return rc;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  if (int rc = decode_begin(ctx, g, batch, kWsFull, h_sizes, stream, &d_sizes)) return rc;
  himg_dev::launch_row_records(g, ctx->dec_ws, batch, (const uint8_t *)d_packed, in_stride, d_sizes, d_status,
                               (hipStream_t)stream, &ctx->prof);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

// ---------------------------------------------------------------------------
// Tensor decode: the planar float output (include/himg_hip.h).  The descriptor is checked on the
// host and rides in the kernel arguments of the store kernels.
// ---------------------------------------------------------------------------
static bool tensor_desc_ok(const himg_hip_tensor_desc *t, int C, himg_dev::TensDesc *td) {
  if (!t || t->dtype < HIMG_DT_F32 || t->dtype > HIMG_DT_BF16 || t->out_channels < 1 || t->out_channels > C || C > 4)
    return false;
  himg_dev::TensDesc d = {};
  d.dtype = t->dtype; d.co = t->out_channels;
  for (int c = 0; c < t->out_channels; ++c) {
    if (!std::isfinite(t->scale[c]) || !std::isfinite(t->bias[c])) return false;
    d.scale[c] = t->scale[c]; d.bias[c] = t->bias[c];
  }
  if (td) *td = d;
  return true;
}

extern "C" int himg_hip_tensor_bytes(const himg_hip_tensor_desc *t, int num_channels, int w, int h,
                                     size_t *bytes_per_frame) {
  Geom g;
  if (!bytes_per_frame || !make_geom(w, h, num_channels, num_channels, 1, &g) || !tensor_desc_ok(t, num_channels, nullptr))
    return HIMG_ERR_ARG;
  *bytes_per_frame = (size_t)t->out_channels * (size_t)h * (size_t)w * (size_t)himg_dev::tens_elem_size(t->dtype);
  return HIMG_OK;
}

extern "C" int himg_hip_decode_tensor_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                             const uint32_t *h_sizes, int batch, int width, int height,
                                             int num_channels, const himg_hip_tensor_desc *t, void *d_out,
                                             int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !t || !d_out || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  himg_dev::TensDesc td;
  const char *bad = tensor_desc_ok(t, num_channels, &td) ? nullptr : "bad tensor descriptor";
  return decode_full(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, d_out, d_status, stream, bad,
                     &td);
}

// ---------------------------------------------------------------------------
// Planes decode: the stream's own channel planes, in front of the colour inverse (include/himg_hip.h).
// The mask is checked on the host and rides in the kernel arguments of the store kernels.
// ---------------------------------------------------------------------------
static bool plane_mask_ok(int C, uint32_t mask) { return C >= 1 && C <= 4 && mask != 0 && (mask >> C) == 0; }

extern "C" int himg_hip_planes_bytes(int num_channels, uint32_t plane_mask, int w, int h, size_t *bytes_per_frame) {
  Geom g;
  if (!bytes_per_frame || !plane_mask_ok(num_channels, plane_mask) || !make_geom(w, h, num_channels, num_channels, 1, &g))
    return HIMG_ERR_ARG;
  *bytes_per_frame = (size_t)himg_dev::plane_count(plane_mask) * (size_t)h * (size_t)w;
  return HIMG_OK;
}

extern "C" int himg_hip_decode_planes_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                             const uint32_t *h_sizes, int batch, int width, int height,
                                             int num_channels, uint32_t plane_mask, void *d_out,
                                             int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_out || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  const himg_dev::PlaneDesc pc = {plane_mask};
  const char *bad = plane_mask_ok(num_channels, plane_mask) ? nullptr : "bad plane mask";
  return decode_full(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, d_out, d_status, stream, bad,
                     &pc);
}

// ---------------------------------------------------------------------------
// Decode into windows of pitched destination pictures (include/himg_hip.h).  The descriptor and the
// origins are checked on the host by the rules of the encoder's source windows (windows_check); the
// descriptor rides in the kernel arguments of the store kernels, the origins with the sizes.
// ---------------------------------------------------------------------------
static const char *dst_check(const himg_hip_dst *dst, int num_channels, int batch, const int32_t *h_origins, int w, int h,
                             size_t *bytes, himg_dev::DstDesc *dd = nullptr) {
  if (!dst) return "bad argument";
  const himg_hip_src s = {dst->width, dst->height, dst->pixel_stride, dst->row_pitch, dst->frame_pitch};
  if (const char *bad = windows_check(&s, num_channels, batch, h_origins, w, h, bytes)) return bad;
  if (dd) { dd->row_pitch = dst->row_pitch; dd->frame_pitch = dst->frame_pitch; dd->org = nullptr; dd->pixel_stride = dst->pixel_stride; }
  return nullptr;
}

extern "C" int himg_hip_dst_extent(const himg_hip_dst *dst, int num_channels, int batch, const int32_t *h_origins,
                                   int w, int h, size_t *bytes) {
  if (!bytes) return HIMG_ERR_ARG;
  *bytes = 0;
  return dst_check(dst, num_channels, batch, h_origins, w, h, bytes) ? HIMG_ERR_ARG : HIMG_OK;
}

extern "C" int himg_hip_decode_into_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                           const uint32_t *h_sizes, int batch, int width, int height,
                                           int num_channels, void *d_dst, const himg_hip_dst *dst,
                                           const int32_t *h_origins, int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_dst || !d_status || batch < 1 || batch > 65535) return HIMG_ERR_ARG;
  himg_dev::DstDesc dd;
  size_t extent = 0;
  const char *bad = dst_check(dst, num_channels, batch, h_origins, width, height, &extent, &dd);
  return decode_full(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, d_dst, d_status, stream, bad,
                     &dd, h_origins);
}

extern "C" int himg_hip_decode_rows_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                           int width, int height, int num_channels, int row0,
                                           int row1, void *d_out_rows, int32_t *d_status,
                                           void *stream) {
  if (!ctx || !d_packed || !d_out_rows || !d_status) return HIMG_ERR_ARG;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, 1, kWsFull, d_packed, d_out_rows, nullptr,
                           bad_row_range(height, row0, row1), &g))
    return rc;
  g.wide_q = wide_q_hint(g, packed_size);
  if (int rc = decode_begin(ctx, g, 1, kWsFull, &packed_size, stream, &d_sizes)) return rc;
  // The kernels address pixel rows of the whole frame; hand them a virtual frame
  // base so that block row row0 lands at the start of d_out_rows.
  uint8_t *base = (uint8_t *)d_out_rows - (size_t)8 * row0 * g.W * g.C;
  launch_decode(g, ctx->dec_ws, 1, (const uint8_t *)d_packed, ((size_t)packed_size + 3) / 4 * 4, d_sizes, base, d_status,
                (hipStream_t)stream, &ctx->prof, ctx->opts, ctx->opts.use_side ? &ctx->dstr : nullptr, row0, row1);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

// Row index of one stream in HBM (rank 0 of a row-sharded decode): container parse and
// the serial row-header walk only.  d_row_index: [rows] payload offsets then [rows]
// lengths; d_rows_first: offset of the first row header (everything in front of it --
// container chunks, LRES stream, FRES tree -- is what every rank needs).
extern "C" int himg_hip_decode_index_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                            int width, int height, int num_channels,
                                            uint32_t *d_row_index, uint32_t *d_rows_first,
                                            int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !d_row_index || !d_rows_first || !d_status) return HIMG_ERR_ARG;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, 1, kWsFull, d_packed, nullptr, nullptr, nullptr, &g))
    return rc;
  if (int rc = decode_begin(ctx, g, 1, kWsFull, &packed_size, stream, &d_sizes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  launch_decode(g, ctx->dec_ws, 1, (const uint8_t *)d_packed, ((size_t)packed_size + 3) / 4 * 4,
                d_sizes, nullptr, d_status, s, &ctx->prof, ctx->opts,
                nullptr, 0, g.rows, nullptr, true);
  HIP_TRY(ctx, hipMemcpyAsync(d_row_index, ctx->dec_ws.row_off, (size_t)g.rows * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(d_row_index + g.rows, ctx->dec_ws.row_len, (size_t)g.rows * 4,
                              hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(d_rows_first, &ctx->dec_ws.frames[0].rows_first, 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

// Block rows [row0, row1) with the row index supplied (no header walk: the buffer
// only has to hold the bytes in front of the first row header and the payloads of
// these rows, each at its offset in the stream).  phase: kDecHead | kDecRows.
static int decode_rows_indexed(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size, int width,
                               int height, int num_channels, int row0, int row1, const uint32_t *d_row_index,
                               void *d_out_rows, int32_t *d_status, void *stream, int phase) {
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, 1, kWsFull, d_packed, d_out_rows, nullptr,
                           bad_row_range(height, row0, row1), &g))
    return rc;
  g.wide_q = wide_q_hint(g, packed_size);
  if (int rc = decode_begin(ctx, g, 1, kWsFull, &packed_size, stream, &d_sizes)) return rc;
  uint8_t *base = d_out_rows ? (uint8_t *)d_out_rows - (size_t)8 * row0 * g.W * g.C : nullptr;
  launch_decode(g, ctx->dec_ws, 1, (const uint8_t *)d_packed, ((size_t)packed_size + 3) / 4 * 4, d_sizes, base, d_status,
                (hipStream_t)stream, &ctx->prof, ctx->opts, ctx->opts.use_side ? &ctx->dstr : nullptr, row0, row1,
                d_row_index, false, phase);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_rows_indexed_device(himg_hip_ctx *ctx, const void *d_packed,
                                                   uint32_t packed_size, int width, int height,
                                                   int num_channels, int row0, int row1,
                                                   const uint32_t *d_row_index, void *d_out_rows,
                                                   int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !d_out_rows || !d_status || !d_row_index) return HIMG_ERR_ARG;
  return decode_rows_indexed(ctx, d_packed, packed_size, width, height, num_channels, row0, row1, d_row_index,
                             d_out_rows, d_status, stream, himg_dev::kDecHead | himg_dev::kDecRows);
}

// The same in two launches, for a rank whose rows' bytes arrive later than the head of
// the stream: decode_head_device needs only the bytes in front of the first row header
// (container parse, LRES chain, predictor inverse: the low-res plane of the whole frame),
// decode_rows_after_head_device -- same context, same stream, same geometry -- the row
// index and the rows' bytes.
extern "C" int himg_hip_decode_head_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                           int width, int height, int num_channels, void *stream) {
  if (!ctx || !d_packed) return HIMG_ERR_ARG;
  const int rc = decode_rows_indexed(ctx, d_packed, packed_size, width, height, num_channels, 0, 0, nullptr, nullptr,
                                     nullptr, stream, himg_dev::kDecHead);
  if (rc == HIMG_OK) {
    ctx->head.valid = true;
    ctx->head.w = width; ctx->head.h = height; ctx->head.c = num_channels;
    ctx->head.packed = d_packed; ctx->head.size = packed_size; ctx->head.stream = stream;
  }
  return rc;
}

extern "C" int himg_hip_decode_rows_after_head_device(himg_hip_ctx *ctx, const void *d_packed,
                                                      uint32_t packed_size, int width, int height,
                                                      int num_channels, int row0, int row1,
                                                      const uint32_t *d_row_index, void *d_out_rows,
                                                      int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !d_out_rows || !d_status || !d_row_index) return HIMG_ERR_ARG;
  const himg_hip_ctx::HeadToken t = ctx->head;
  if (!t.valid)
    return fail(ctx, HIMG_ERR_ARG, "decode_rows_after_head_device: no decode_head_device in front of it (or another decode since)");
  if (t.w != width || t.h != height || t.c != num_channels || t.packed != d_packed || t.size != packed_size ||
      t.stream != stream)
    return fail(ctx, HIMG_ERR_ARG, "decode_rows_after_head_device: not the stream / geometry / HIP stream of decode_head_device");
  const int rc = decode_rows_indexed(ctx, d_packed, packed_size, width, height, num_channels, row0, row1, d_row_index,
                                     d_out_rows, d_status, stream, himg_dev::kDecRows);
  if (rc == HIMG_OK) ctx->head = t;   // (another row range of the same frame may follow)
  return rc;
}

// The row index of a stream in HBM by the header walk ALONE (k_dec_rowwalk finds the FRES
// payload itself), on the context's side stream behind whatever `stream` holds at the time of
// the call: launched in front of decode_head_device it runs BESIDE the head phase (they
// touch disjoint fields, as in every decode).  Results arrive with
// himg_hip_decode_walk_wait: d_row_index ([rows] offsets, [rows] lengths), d_rows_first,
// d_status (the walk's verdict only; the container's is the head phase's).
extern "C" int himg_hip_decode_walk_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                           int width, int height, int num_channels, uint32_t *d_row_index,
                                           uint32_t *d_rows_first, int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !d_row_index || !d_rows_first || !d_status) return HIMG_ERR_ARG;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, 1, kWsFull, d_packed, nullptr, nullptr, nullptr, &g))
    return rc;
  if (int rc = decode_begin(ctx, g, 1, kWsFull, &packed_size, stream, &d_sizes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipStream_t w = ctx->opts.use_side ? ctx->dstr.side : s;
  if (w != s) {
    HIP_TRY(ctx, hipEventRecord(ctx->dstr.ev_fork, s));
    HIP_TRY(ctx, hipStreamWaitEvent(w, ctx->dstr.ev_fork, 0));
  }
  himg_dev::launch_rowwalk_only(g, ctx->dec_ws, (const uint8_t *)d_packed, ((size_t)packed_size + 3) / 4 * 4,
                                d_sizes, w);
  HIP_TRY(ctx, hipMemcpyAsync(d_row_index, ctx->dec_ws.row_off, (size_t)g.rows * 4, hipMemcpyDeviceToDevice, w));
  HIP_TRY(ctx, hipMemcpyAsync(d_row_index + g.rows, ctx->dec_ws.row_len, (size_t)g.rows * 4, hipMemcpyDeviceToDevice, w));
  HIP_TRY(ctx, hipMemcpyAsync(d_rows_first, &ctx->dec_ws.frames[0].rows_first, 4, hipMemcpyDeviceToDevice, w));
  HIP_TRY(ctx, hipMemcpyAsync(d_status, &ctx->dec_ws.frames[0].walk_status, 4, hipMemcpyDeviceToDevice, w));
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_walk_ranges_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                                  int width, int height, int num_channels, const int *range_end,
                                                  int n_ranges, uint32_t *d_row_index, uint32_t *d_rows_first,
                                                  int32_t *d_range_status, void *stream) {
  if (!ctx || !d_packed || !d_row_index || !d_rows_first || !d_range_status || !range_end || n_ranges < 1 ||
      n_ranges > HIMG_MAX_WALK_RANGES)
    return HIMG_ERR_ARG;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, 1, kWsFull, d_packed, nullptr, nullptr, nullptr, &g))
    return rc;
  for (int k = 0; k < n_ranges; ++k)
    if (range_end[k] < 0 || (k && range_end[k] < range_end[k - 1])) return fail(ctx, HIMG_ERR_ARG, "range ends must ascend");
  if (int rc = decode_begin(ctx, g, 1, kWsFull, &packed_size, stream, &d_sizes)) return rc;
  for (int k = 0; k < n_ranges; ++k)
    if (!ctx->ev_range[k]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_range[k], hipEventDisableTiming));
  hipStream_t s = (hipStream_t)stream;
  hipStream_t w = ctx->opts.use_side ? ctx->dstr.side : s;
  if (w != s) {
    HIP_TRY(ctx, hipEventRecord(ctx->dstr.ev_fork, s));
    HIP_TRY(ctx, hipStreamWaitEvent(w, ctx->dstr.ev_fork, 0));
  }
  int done = 0;   // rows whose index entries have been copied out
  for (int k = 0; k < n_ranges; ++k) {
    const bool last = k + 1 == n_ranges || range_end[k] >= g.rows;
    const int upto = last ? g.rows : range_end[k];
    himg_dev::launch_rowwalk_range(g, ctx->dec_ws, (const uint8_t *)d_packed, ((size_t)packed_size + 3) / 4 * 4,
                                   d_sizes, last ? 0x7fffffff : upto, k > 0, w);
    if (upto > done) {
      HIP_TRY(ctx, hipMemcpyAsync(d_row_index + done, ctx->dec_ws.row_off + done, (size_t)(upto - done) * 4, hipMemcpyDeviceToDevice, w));
      HIP_TRY(ctx, hipMemcpyAsync(d_row_index + g.rows + done, ctx->dec_ws.row_len + done, (size_t)(upto - done) * 4, hipMemcpyDeviceToDevice, w));
      done = upto;
    }
    if (k == 0) HIP_TRY(ctx, hipMemcpyAsync(d_rows_first, &ctx->dec_ws.frames[0].rows_first, 4, hipMemcpyDeviceToDevice, w));
    HIP_TRY(ctx, hipMemcpyAsync(d_range_status + k, &ctx->dec_ws.frames[0].walk_status, 4, hipMemcpyDeviceToDevice, w));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_range[k], w));
    ctx->n_ranges = k + 1;
    if (last) {   // (ranges behind the last row: nothing left to walk; their events are this one)
      for (int j = k + 1; j < n_ranges; ++j) {
        HIP_TRY(ctx, hipMemcpyAsync(d_range_status + j, &ctx->dec_ws.frames[0].walk_status, 4, hipMemcpyDeviceToDevice, w));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_range[j], w));
      }
      ctx->n_ranges = n_ranges;
      break;
    }
  }
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_walk_wait_range(himg_hip_ctx *ctx, int k) {
  if (!ctx || k < 0 || k >= ctx->n_ranges || !ctx->ev_range[k]) return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_range[k]));
  return HIMG_OK;
}

extern "C" int himg_hip_decode_walk_wait(himg_hip_ctx *ctx) {
  if (!ctx) return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (without a side stream the walk went to the caller's stream)
  HIP_TRY(ctx, hipStreamSynchronize(ctx->opts.use_side ? ctx->dstr.side : ctx->last_stream));
  return HIMG_OK;
}

// Where the first FRES row header lies (container parse + the length of the serialised
// tree, no header walk): what the rank that holds a stream in HBM needs to send the head
// of the stream on its way before it indexes the rows.
extern "C" int himg_hip_decode_first_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                            int width, int height, int num_channels, uint32_t *d_rows_first,
                                            int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !d_rows_first || !d_status) return HIMG_ERR_ARG;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, 1, kWsFull, d_packed, nullptr, nullptr, nullptr, &g))
    return rc;
  if (int rc = decode_begin(ctx, g, 1, kWsFull, &packed_size, stream, &d_sizes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  launch_decode(g, ctx->dec_ws, 1, (const uint8_t *)d_packed, ((size_t)packed_size + 3) / 4 * 4,
                d_sizes, nullptr, d_status, s, &ctx->prof, ctx->opts,
                nullptr, 0, 0, nullptr, true);
  HIP_TRY(ctx, hipMemcpyAsync(d_rows_first, &ctx->dec_ws.frames[0].rows_first, 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

// The same index on the host, for a stream in host memory (no GPU): chunk search
// (decoder.cpp:428-461), length of the serialised FRES tree (huffman_dec.cpp:152-229),
// row headers (huffman_dec.cpp:232-248).  A serial walk over a few thousand headers is
// microseconds on a CPU and 1 ms of dependent loads on the GPU.
static bool host_find_chunk(const uint8_t *p, size_t n, size_t *idx, uint32_t tag, uint32_t *size) {
  for (;;) {
    if (*idx + 8 > n) return false;
    uint32_t t, sz;
    memcpy(&t, p + *idx, 4);
    memcpy(&sz, p + *idx + 4, 4);
    *idx += 8;
    if (sz > 0x7fffffffu || *idx + sz > n) return false;
    if (t == tag) { *size = sz; return true; }
    *idx += sz;
  }
}

// The walk behind every host index and region plan: the chunk search to FRES, the length of the
// serialised tree, then the row headers of rows 0 .. row1-1 (to the end of the chunk when row1 is the
// last row: the reference's Init walks them all).  plan: head_bytes, and rows_begin / rows_end of rows
// row0 .. row1-1; row_index (2 x rows words, or nullptr): their offsets and lengths.
static int host_walk(const uint8_t *packed, size_t packed_size, int fix_t2, int rows, int row0, int row1,
                     himg_hip_region_plan *plan, uint32_t *row_index) {
  static const uint32_t tags[6] = {0x544d5246u, 0x50414d4cu, 0x5345524cu, 0x47464351u, 0x50414d46u, 0x53455246u};
  size_t idx = 12;
  uint32_t sz = 0;
  for (int t = 0; t < 6; ++t) {
    if (!host_find_chunk(packed, packed_size, &idx, tags[t], &sz)) return HIMG_ERR_FORMAT;
    if (t < 5) idx += sz;
  }
  const size_t coff = idx, end = idx + sz;
  size_t bit = 0;
  {
    const size_t bit_end = 8 * (size_t)(sz < (uint32_t)kTreeStride ? sz : (uint32_t)kTreeStride);
    int open = 1, count = 0;
    while (open > 0) {
      if (count >= 2 * kNumSym - 1 || bit >= bit_end) return HIMG_ERR_FORMAT;
      ++count;
      if ((packed[coff + (bit >> 3)] >> (bit & 7)) & 1) {
        if (bit + 10 > bit_end) return HIMG_ERR_FORMAT;
        bit += 10;
        --open;
      } else {
        bit += 1;
        ++open;
      }
    }
  }
  size_t q = coff + ((bit + 7) >> 3);
  if (q >= end) return HIMG_ERR_FORMAT;
  plan->head_bytes = q;
  if (fix_t2 && rows == 1) {   // one block row without a size header
    plan->rows_begin = q; plan->rows_end = end;
    if (row_index) { row_index[0] = (uint32_t)q; row_index[rows] = (uint32_t)(end - q); }
    return HIMG_OK;
  }
  int r = 0;
  while (q != end && (r < row1 || row1 == rows)) {
    if (q + 2 > end) return HIMG_ERR_FORMAT;
    const size_t hdr = q;
    uint32_t len = packed[q] | (packed[q + 1] << 8);
    q += 2;
    if (len & 0x8000u) {
      if (q + 2 > end) return HIMG_ERR_FORMAT;
      len = (len & 0x7fffu) | ((uint32_t)(packed[q] | (packed[q + 1] << 8)) << 15);
      q += 2;
    }
    if (len > end - q) return HIMG_ERR_FORMAT;
    if (r == row0) plan->rows_begin = hdr;
    if (r == row1 - 1) plan->rows_end = q + len;
    if (row_index && r >= row0 && r < row1) { row_index[r] = (uint32_t)q; row_index[rows + r] = len; }
    ++r;
    q += len;
  }
  return r < row1 || (row1 == rows && r < rows) ? HIMG_ERR_FORMAT : HIMG_OK;
}

extern "C" int himg_hip_index_host(const uint8_t *packed, size_t packed_size, int fix_t2, int *width,
                                   int *height, int *num_channels, uint32_t *row_index,
                                   size_t index_rows, uint32_t *rows_first) {
  if (!packed || !width || !height || !num_channels || !rows_first) return HIMG_ERR_ARG;
  int rc = himg_hip_peek(packed, packed_size, width, height, num_channels);
  if (rc) return rc;
  const int rows = (*height + 7) / 8;
  if (!row_index || index_rows < (size_t)rows) return HIMG_ERR_CAPACITY;
  himg_hip_region_plan plan = himg_hip_region_plan();
  rc = host_walk(packed, packed_size, fix_t2, rows, 0, rows, &plan, row_index);   // (the whole frame)
  if (plan.head_bytes) *rows_first = (uint32_t)plan.head_bytes;
  return rc;
}

// ---------------------------------------------------------------------------
// Host-buffer API.
// ---------------------------------------------------------------------------
// ---- host-buffer API ---------------------------------------------------------
// The stream / the pixels of the last host call stay resident in ctx->h_out; the
// entry points differ only in where they copy them to.

// What a host encode form asks for, for each of its frames.
enum HostEncKind { kEncPlain, kEncBudget, kEncTarget, kEncWindow };
struct HostEncReq {
  HostEncKind kind;
  int quality;               // kEncPlain
  int qmin, qmax;            // the searches: the range, each frame's limit, and where the chosen quality goes
  const size_t *budgets;     // kEncBudget  (-1 for a frame whose budget is below its size at qmin)
  const uint64_t *max_sse;   // kEncTarget  (-1 for a frame that misses its target at qmax)
  int *qualities;
  uint64_t *sses;            // kEncTarget: where the sse reached goes
  const himg_hip_src *src;   // kEncWindow (with `quality`): the host picture, and the window's origin in it --
  int x, y;                  // the width and height of the call are the window's
};
static bool req_range_ok(himg_hip_ctx *ctx, const HostEncReq &rq) {
  if (himg_hip_budget_probes(rq.qmin, rq.qmax) >= 0) return true;
  fail(ctx, HIMG_ERR_ARG, "the quality range must satisfy 0 <= qmin <= qmax <= 100");
  return false;
}
// The device form of the request for its frame i (at d_in, one frame), the results to *d_res.
static int encode_request_device(himg_hip_ctx *ctx, const HostEncReq &rq, int i, const void *d_in, int width, int height,
                                 int pixel_stride, int num_channels, int use_ycbcr, void *d_out, size_t cap,
                                 HostResult *d_res, hipStream_t s) {
  switch (rq.kind) {
    case kEncBudget: {
      const uint32_t b = rq.budgets[i] > 0xffffffffull ? 0xffffffffu : (uint32_t)rq.budgets[i];
      return himg_hip_encode_budget_device(ctx, d_in, 1, width, height, pixel_stride, num_channels, rq.qmin, rq.qmax,
                                           use_ycbcr, &b, d_out, cap, &d_res->size, &d_res->quality, &d_res->status, s);
    }
    case kEncTarget:
      return himg_hip_encode_target_device(ctx, d_in, 1, width, height, pixel_stride, num_channels, rq.qmin, rq.qmax,
                                           use_ycbcr, rq.max_sse + i, d_out, cap, &d_res->size, &d_res->quality,
                                           &d_res->sse, &d_res->status, s);
    case kEncWindow: {
      // (d_in: the source's rows [y, y + height), so the window begins in its first row)
      const himg_hip_src rows = {rq.src->width, height, pixel_stride, rq.src->row_pitch, 0};
      const int32_t org[2] = {rq.x, 0};
      return himg_hip_encode_windows_device(ctx, d_in, &rows, 1, num_channels, org, width, height, &rq.quality, use_ycbcr,
                                            d_out, cap, &d_res->size, &d_res->status, s);
    }
    default:
      return himg_hip_encode_device(ctx, d_in, 1, width, height, pixel_stride, num_channels, rq.quality, use_ycbcr, d_out,
                                    cap, &d_res->size, &d_res->status, s);
  }
}
// Frame i's results to where the request wants them, and its status as the host API reports it.
static int encode_verdict(himg_hip_ctx *ctx, const HostEncReq &rq, int i, const HostResult &r) {
  if (rq.kind == kEncBudget || rq.kind == kEncTarget) rq.qualities[i] = r.quality;
  if (rq.kind == kEncTarget) rq.sses[i] = r.sse;
  if (rq.kind == kEncTarget && r.status == HIMG_ERR_TARGET)
    return fail(ctx, HIMG_ERR_TARGET, "the distortion at qmax is above the target");
  if (rq.kind == kEncBudget && r.status == HIMG_ERR_CAPACITY)
    return fail(ctx, HIMG_ERR_CAPACITY, "the budget is below the stream's size at qmin");
  if (r.status) return fail(ctx, status_to_code(r.status), "device encode reported an error");
  return HIMG_OK;
}

static int encode_core(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                       int pixel_stride, int num_channels, int use_ycbcr, const HostEncReq &rq, uint32_t *n_out) {
  Geom g;
  if (!make_geom(width, height, pixel_stride, num_channels, use_ycbcr, &g))
    return fail(ctx, HIMG_ERR_ARG, "bad geometry");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t cap = himg_hip_max_packed_size(width, height, num_channels);
  // What goes up: the frame; of a window's source the rows it lies in, up to its last pixel.
  size_t in_bytes = (size_t)g.frame_bytes;
  if (rq.kind == kEncWindow) {
    himg_hip_src one = *rq.src;
    one.frame_pitch = 0;   // (one picture: the descriptor's is ignored)
    const int32_t org[2] = {rq.x, rq.y};
    size_t end = 0;
    if (const char *bad = windows_check(&one, num_channels, 1, org, width, height, &end)) return fail(ctx, HIMG_ERR_ARG, bad);
    data += (size_t)rq.y * rq.src->row_pitch;
    in_bytes = end - (size_t)rq.y * rq.src->row_pitch;
  }
  if (!ctx->h_in.reserve(round_up(in_bytes, 256)) || !ctx->h_out.reserve(cap) ||
      !ctx->h_result.reserve(256))
    return fail(ctx, HIMG_ERR_HIP, "staging allocation failed");
  ctx->host_bytes = 0;
  HIP_TRY(ctx, hipMemcpy(ctx->h_in.p, data, in_bytes, hipMemcpyHostToDevice));
  int rc = encode_request_device(ctx, rq, 0, ctx->h_in.p, width, height, pixel_stride, num_channels, use_ycbcr,
                                 ctx->h_out.p, cap, (HostResult *)ctx->h_result.p, nullptr);
  if (rc) return rc;
  HostResult r = {};
  HIP_TRY(ctx, hipMemcpy(&r, ctx->h_result.p, sizeof(r), hipMemcpyDeviceToHost));
  if ((rc = encode_verdict(ctx, rq, 0, r))) return rc;
  ctx->host_bytes = r.size;
  *n_out = r.size;
  return HIMG_OK;
}

extern "C" int himg_hip_encode(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                               int pixel_stride, int num_channels, int quality, int use_ycbcr,
                               uint8_t **out, size_t *out_size) {
  if (!ctx || !data || !out || !out_size) return HIMG_ERR_ARG;
  *out = nullptr;
  *out_size = 0;
  uint32_t n = 0;
  const HostEncReq rq = {kEncPlain, quality};
  const int rc = encode_core(ctx, data, width, height, pixel_stride, num_channels, use_ycbcr, rq, &n);
  if (rc) return rc;
  uint8_t *buf = (uint8_t *)std::malloc(n ? n : 1);
  if (!buf) return fail(ctx, HIMG_ERR_ARG, "out of host memory");
  HIP_TRY(ctx, hipMemcpy(buf, ctx->h_out.p, n, hipMemcpyDeviceToHost));
  *out = buf;
  *out_size = n;
  return HIMG_OK;
}

// The `_to` forms: the encode, then the size, and the stream where dst has room for it.
static int encode_to(himg_hip_ctx *ctx, const uint8_t *data, int width, int height, int pixel_stride, int num_channels,
                     int use_ycbcr, const HostEncReq &rq, uint8_t *dst, size_t dst_cap, size_t *out_size) {
  if ((rq.kind == kEncBudget || rq.kind == kEncTarget) && !req_range_ok(ctx, rq)) return HIMG_ERR_ARG;
  uint32_t n = 0;
  const int rc = encode_core(ctx, data, width, height, pixel_stride, num_channels, use_ycbcr, rq, &n);
  if (rc) return rc;
  *out_size = n;
  if (!dst || dst_cap < n) return fail(ctx, HIMG_ERR_CAPACITY, "output buffer too small");
  HIP_TRY(ctx, hipMemcpy(dst, ctx->h_out.p, n, hipMemcpyDeviceToHost));
  return HIMG_OK;
}

extern "C" int himg_hip_encode_to(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                                  int pixel_stride, int num_channels, int quality, int use_ycbcr,
                                  uint8_t *dst, size_t dst_cap, size_t *out_size) {
  if (!ctx || !data || !out_size) return HIMG_ERR_ARG;
  *out_size = 0;
  const HostEncReq rq = {kEncPlain, quality};
  return encode_to(ctx, data, width, height, pixel_stride, num_channels, use_ycbcr, rq, dst, dst_cap, out_size);
}

extern "C" int himg_hip_encode_window_to(himg_hip_ctx *ctx, const uint8_t *data, const himg_hip_src *src, int num_channels,
                                         int x, int y, int w, int h, int quality, int use_ycbcr, uint8_t *dst,
                                         size_t dst_cap, size_t *out_size) {
  if (!ctx || !data || !out_size) return HIMG_ERR_ARG;
  *out_size = 0;
  if (!src) return fail(ctx, HIMG_ERR_ARG, "bad argument");
  const HostEncReq rq = {kEncWindow, quality, 0, 0, nullptr, nullptr, nullptr, nullptr, src, x, y};
  return encode_to(ctx, data, w, h, src->pixel_stride, num_channels, use_ycbcr, rq, dst, dst_cap, out_size);
}

extern "C" int himg_hip_encode_budget_to(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                                         int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                                         size_t budget, uint8_t *dst, size_t dst_cap, size_t *out_size, int *quality) {
  if (!ctx || !data || !out_size || !quality) return HIMG_ERR_ARG;
  *out_size = 0;
  *quality = -1;
  const HostEncReq rq = {kEncBudget, 0, qmin, qmax, &budget, nullptr, quality, nullptr};
  return encode_to(ctx, data, width, height, pixel_stride, num_channels, use_ycbcr, rq, dst, dst_cap, out_size);
}

extern "C" int himg_hip_encode_target_to(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                                         int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                                         uint64_t max_sse, uint8_t *dst, size_t dst_cap, size_t *out_size, int *quality,
                                         uint64_t *sse) {
  if (!ctx || !data || !out_size || !quality || !sse) return HIMG_ERR_ARG;
  *out_size = 0;
  *quality = -1;
  *sse = 0;
  const HostEncReq rq = {kEncTarget, 0, qmin, qmax, nullptr, &max_sse, quality, sse};
  return encode_to(ctx, data, width, height, pixel_stride, num_channels, use_ycbcr, rq, dst, dst_cap, out_size);
}

// Geometry from the FRMT chunk (decoder.cpp:144-200).  Returns nullptr or the
// reference's message for the failing check.
static const char *parse_header(const uint8_t *packed, size_t packed_size, int *W, int *H, int *C, int *cs = nullptr) {
  // decoder.cpp:144-166: the RIFF size field must match the buffer exactly.
  if (packed_size < 12 || packed_size > 0x7fffffffu || memcmp(packed, "RIFF", 4) != 0 ||
      memcmp(packed + 8, "HIMG", 4) != 0 ||
      (size_t)(packed[4] | (packed[5] << 8) | (packed[6] << 16) | ((uint32_t)packed[7] << 24)) + 8 != packed_size)
    return "Not a RIFF HIMG file.\n";
  size_t idx = 12;
  for (;;) {
    if (idx + 8 > packed_size) return "Error decoding header.\n";
    const uint32_t sz = packed[idx + 4] | (packed[idx + 5] << 8) | (packed[idx + 6] << 16) |
                        ((uint32_t)packed[idx + 7] << 24);
    const bool frmt = memcmp(packed + idx, "FRMT", 4) == 0;
    idx += 8;
    if (idx + sz > packed_size) return "Error decoding header.\n";
    if (frmt) {
      if (sz < 11 || packed[idx] != 1) return "Error decoding header.\n";
      *W = (int)(packed[idx + 1] | (packed[idx + 2] << 8) | (packed[idx + 3] << 16) | ((uint32_t)packed[idx + 4] << 24));
      *H = (int)(packed[idx + 5] | (packed[idx + 6] << 8) | (packed[idx + 7] << 16) | ((uint32_t)packed[idx + 8] << 24));
      *C = packed[idx + 9];
      if (cs) *cs = packed[idx + 10];
      return nullptr;
    }
    idx += sz;
  }
}

extern "C" int himg_hip_peek(const uint8_t *packed, size_t packed_size, int *width, int *height,
                             int *num_channels) {
  if (!packed || !width || !height || !num_channels) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  if (parse_header(packed, packed_size, &W, &H, &C)) return HIMG_ERR_FORMAT;
  // The FRMT fields are untrusted: callers size their output from them, so apply
  // the engine's limits (make_geom) before anybody allocates.
  Geom g;
  if (!make_geom(W, H, C, C, 1, &g)) return HIMG_ERR_UNSUPPORTED;
  *width = W; *height = H; *num_channels = C;
  return HIMG_OK;
}

extern "C" int himg_hip_peek_format(const uint8_t *packed, size_t packed_size, int *width, int *height,
                                    int *num_channels, int *colour_space) {
  if (!packed || !width || !height || !num_channels || !colour_space) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0, cs = 0;
  if (parse_header(packed, packed_size, &W, &H, &C, &cs)) return HIMG_ERR_FORMAT;
  Geom g;   // (the engine's limits, as in himg_hip_peek)
  if (!make_geom(W, H, C, C, 1, &g)) return HIMG_ERR_UNSUPPORTED;
  *width = W; *height = H; *num_channels = C; *colour_space = cs;
  return HIMG_OK;
}

// What the host entry points check of a stream (nullptr: a batch's missing one) before they plan its
// decode: the header, with the reference's message, and the engine's limits.  The host only needs the
// geometry to size the launch; every check is repeated on the device (k_dec_parse).
static int stream_geom(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int *W, int *H, int *C, Geom *g) {
  if (const char *msg = packed ? parse_header(packed, packed_size, W, H, C) : "Not a RIFF HIMG file.\n")
    return fail(ctx, HIMG_ERR_FORMAT, msg);
  if (!make_geom(*W, *H, *C, *C, 1, g)) return fail(ctx, HIMG_ERR_UNSUPPORTED, "unsupported geometry");
  return HIMG_OK;
}

// ---- The steps the host decodes of one stream share: the staging reserved, the stream and the host's row
// index up, the verdict behind the launch read, the result delivered.  Everything is ordered on the null
// stream, which the decode runs on; the one wait of a call is the read of its verdict.  (What each entry
// point does with them: DESIGN.md, "The host decodes' contract".)
// The slot of a stream of n bytes in the staging: the row kernels read whole dwords and a few dwords
// ahead, so a slot ends at least 16 bytes behind its stream.
static size_t stage_slot(size_t n) { return round_up(n + 16, 256); }

// A call's staging, on the context's device: in_bytes of `in` (h_in, or a buffer that becomes a handle's), out_bytes of h_out,
// status_bytes of h_status, and n_idx dwords of h_index with the pinned hp_index they go up from (the
// context keeps it: a call returns only after the decode that reads its copy has finished).  A call that
// takes h_out leaves nothing there for himg_hip_fetch_last until it says so.
static int stage_reserve(himg_hip_ctx *ctx, DevBuf &in, size_t in_bytes, size_t out_bytes, size_t status_bytes,
                         size_t n_idx) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (out_bytes) ctx->host_bytes = 0;
  if (!in.reserve(in_bytes) || !ctx->h_out.reserve(round_up(out_bytes, 256)) ||
      !ctx->h_status.reserve(round_up(status_bytes, 256)) || !ctx->h_index.reserve(round_up(n_idx * 4, 256)))
    return fail(ctx, HIMG_ERR_HIP, "staging allocation failed");
  if (ctx->hp_index_cap >= n_idx) return HIMG_OK;
  if (ctx->hp_index) hipHostFree(ctx->hp_index);
  ctx->hp_index = nullptr; ctx->hp_index_cap = 0;
  if (hipHostMalloc((void **)&ctx->hp_index, round_up(n_idx * 4, 4096), hipHostMallocDefault) != hipSuccess)
    return fail(ctx, HIMG_ERR_HIP, "pinned index allocation failed");
  ctx->hp_index_cap = round_up(n_idx * 4, 4096) / 4;
  return HIMG_OK;
}

// A stream (or its first n bytes) into the staging slot [d, d + slot): the row kernels read whole dwords
// and a few dwords ahead, so nothing of a stream staged before may lie behind this one -- zeros from
// the last 16-byte boundary to the end of the slot, then the bytes.  With ranges (n_ranges pairs of
// begin, end) only those bytes go up, each at its offset: the head and the rows a plan touches, beside
// which the kernels, led by the host's index, read nothing.
static int stage_upload(himg_hip_ctx *ctx, uint8_t *d, size_t slot, const uint8_t *src, size_t n,
                        const size_t *ranges = nullptr, size_t n_ranges = 0) {
  if (!ranges) {
    HIP_TRY(ctx, hipMemsetAsync(d + (n & ~(size_t)15), 0, slot - (n & ~(size_t)15), nullptr));
    HIP_TRY(ctx, hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, nullptr));
  }
  for (size_t i = 0; i < n_ranges; ++i)
    if (ranges[2 * i + 1] > ranges[2 * i])
      HIP_TRY(ctx, hipMemcpyAsync(d + ranges[2 * i], src + ranges[2 * i], ranges[2 * i + 1] - ranges[2 * i],
                                  hipMemcpyHostToDevice, nullptr));
  return HIMG_OK;
}

// The host's row index, n_idx dwords that a caller's walk left in hp_index, into h_index.
static int stage_index(himg_hip_ctx *ctx, size_t n_idx) {
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_index.p, ctx->hp_index, n_idx * 4, hipMemcpyHostToDevice, nullptr));
  return HIMG_OK;
}

// The two steps of a host form that sends one stream (its first n bytes) up whole, for the device to walk.
static int stage_whole(himg_hip_ctx *ctx, const uint8_t *packed, size_t n, size_t out_bytes, size_t status_bytes) {
  if (int rc = stage_reserve(ctx, ctx->h_in, stage_slot(n), out_bytes, status_bytes, 0)) return rc;
  return stage_upload(ctx, (uint8_t *)ctx->h_in.p, stage_slot(n), packed, n);
}

// The verdict behind a launch: launch_rc is what the device entry point returned.  A refused launch is
// waited for, because the uploads may still be reading the caller's and the pinned buffers.  Else the
// first n words of h_status come down to st.  what == nullptr: a batch's, which its caller judges frame by
// frame.  statuses == nullptr: st[0] is the call's status word (the words behind it are results of the
// entry point's own) and `what` the message of a status that has no text of the reference's -- what_arg,
// where given, for one that blames an argument.  Else the words are n windows': each one's code to
// statuses, the first failing window's message the call's (the windows' failures are no failure of this
// step: the call delivers what the others decoded and returns first_code).
static int stage_verdict(himg_hip_ctx *ctx, int launch_rc, int32_t *st, size_t n, const char *what = kDecodeError,
                         int *statuses = nullptr, const char *what_arg = nullptr) {
  if (launch_rc) return (void)hipStreamSynchronize(nullptr), launch_rc;
  HIP_TRY(ctx, hipMemcpy(st, ctx->h_status.p, n * 4, hipMemcpyDeviceToHost));
  if (!what) return HIMG_OK;
  if (!statuses)
    return st[0] ? status_error(ctx, st[0], what_arg && status_to_code(st[0]) == HIMG_ERR_ARG ? what_arg : what) : HIMG_OK;
  for (size_t k = n; k-- > 0;) {   // (backwards: the message left is the first failing window's)
    statuses[k] = status_to_code(st[k]);
    if (st[k]) (void)status_error(ctx, st[k], what);
  }
  return HIMG_OK;
}

// What a call of n windows returns behind its delivery: the first failing window's code.
static int first_code(const int *statuses, int n) {
  for (int k = 0; k < n; ++k)
    if (statuses[k]) return statuses[k];
  return HIMG_OK;
}

// A piece of the output staging and the caller's buffer it goes to.
struct Piece { size_t at, bytes; uint8_t *dst; size_t cap; };

// The capacity rule: every piece has a buffer that holds it.
static int pieces_fit(himg_hip_ctx *ctx, const Piece *pc, int n) {
  for (int i = 0; i < n; ++i)
    if (!pc[i].dst || pc[i].cap < pc[i].bytes) return fail(ctx, HIMG_ERR_CAPACITY, "output buffer too small");
  return HIMG_OK;
}

static int pieces_copy(himg_hip_ctx *ctx, const Piece *pc, int n) {
  for (int i = 0; i < n; ++i)
    if (pc[i].bytes)
      HIP_TRY(ctx, hipMemcpy(pc[i].dst, (const uint8_t *)ctx->h_out.p + pc[i].at, pc[i].bytes, hipMemcpyDeviceToHost));
  return HIMG_OK;
}

// What a call reports before it copies: the dimensions, then the capacity rule -- so a caller whose
// buffer is too small learns what to allocate.
static int out_check(himg_hip_ctx *ctx, int W, int H, int C, int *width, int *height, int *channels, const Piece *pc,
                     int n) {
  *width = W; *height = H; *channels = C;
  return pieces_fit(ctx, pc, n);
}

// The delivery behind a good verdict: `resident` bytes of h_out stay for himg_hip_fetch_last (0: none),
// out_check, the copies.  (The entry points that check the capacity before they launch call out_check
// there and pieces_copy here.)
static int deliver(himg_hip_ctx *ctx, int W, int H, int C, int *width, int *height, int *channels, size_t resident,
                   const Piece *pc, int n) {
  ctx->host_bytes = resident;
  if (int rc = out_check(ctx, W, H, C, width, height, channels, pc, n)) return rc;
  return pieces_copy(ctx, pc, n);
}

extern "C" int himg_hip_fetch_last(himg_hip_ctx *ctx, uint8_t *dst, size_t dst_cap, size_t *size) {
  if (!ctx || !size) return HIMG_ERR_ARG;
  *size = ctx->host_bytes;
  if (!ctx->host_bytes) return fail(ctx, HIMG_ERR_ARG, "no result to fetch");
  const Piece pc = {0, ctx->host_bytes, dst, dst_cap};
  if (int rc = pieces_fit(ctx, &pc, 1)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return pieces_copy(ctx, &pc, 1);
}

static int decode_core(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int *W, int *H,
                       int *C) {
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, W, H, C, &g)) return rc;
  const size_t in_cap = stage_slot(packed_size), out_bytes = (size_t)*W * *H * *C;
  const size_t n_idx = g.rows >= 2 ? 2 * (size_t)g.rows : 0;
  if (int rc = stage_reserve(ctx, ctx->h_in, in_cap, out_bytes, 4, n_idx)) return rc;
  // The stream is in host memory: the FRES rows are indexed HERE -- the walk over the row
  // size headers (huffman_dec.cpp:232-248) is a chain of dependent reads, microseconds on
  // a CPU and 0.24 ms of a 0.41 ms decode as k_dec_rowwalk's 512 dependent HBM loads -- and
  // the index goes up with the stream.  A stream the host walk does not accept (damaged headers, a
  // geometry it does not index) takes the device walk, which words the verdict.
  if (int rc = stage_upload(ctx, (uint8_t *)ctx->h_in.p, in_cap, packed, packed_size)) return rc;
  const uint32_t sz32 = (uint32_t)packed_size;
  int rc = -1;
  uint32_t first = 0;
  int w2 = 0, h2 = 0, c2 = 0;
  if (n_idx && himg_hip_index_host(packed, packed_size, ctx->fix_t2, &w2, &h2, &c2, ctx->hp_index, (size_t)g.rows, &first) == HIMG_OK) {
    if (int e = stage_index(ctx, n_idx)) return e;
    rc = himg_hip_decode_rows_indexed_device(ctx, ctx->h_in.p, sz32, *W, *H, *C, 0, g.rows, (const uint32_t *)ctx->h_index.p,
                                             ctx->h_out.p, (int32_t *)ctx->h_status.p, nullptr);
  }
  if (rc == -1)
    rc = himg_hip_decode_device(ctx, ctx->h_in.p, in_cap, &sz32, 1, *W, *H, *C, ctx->h_out.p,
                                (int32_t *)ctx->h_status.p, nullptr);
  int32_t st = 0;
  if ((rc = stage_verdict(ctx, rc, &st, 1))) return rc;
  ctx->host_bytes = out_bytes;   // (resident: the three callers copy it down each in their own way)
  return HIMG_OK;
}

extern "C" int himg_hip_decode(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                               uint8_t **out, int *width, int *height, int *num_channels) {
  if (!ctx || !packed || !out || !width || !height || !num_channels) return HIMG_ERR_ARG;
  *out = nullptr;
  int W = 0, H = 0, C = 0;
  const int rc = decode_core(ctx, packed, packed_size, &W, &H, &C);
  if (rc) return rc;
  const size_t out_bytes = ctx->host_bytes;
  uint8_t *buf = (uint8_t *)std::malloc(out_bytes ? out_bytes : 1);
  if (!buf) return fail(ctx, HIMG_ERR_ARG, "out of host memory");
  HIP_TRY(ctx, hipMemcpy(buf, ctx->h_out.p, out_bytes, hipMemcpyDeviceToHost));
  *out = buf;
  *width = W; *height = H; *num_channels = C;
  return HIMG_OK;
}

extern "C" int himg_hip_decode_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                                  uint8_t *dst, size_t dst_cap, int *width, int *height,
                                  int *num_channels) {
  if (!ctx || !packed || !width || !height || !num_channels) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  const int rc = decode_core(ctx, packed, packed_size, &W, &H, &C);
  if (rc) return rc;
  const Piece pc = {0, ctx->host_bytes, dst, dst_cap};
  return deliver(ctx, W, H, C, width, height, num_channels, ctx->host_bytes, &pc, 1);
}

// The whole picture of a host stream into a host picture at (x, y): himg_hip_decode_to's decode, then
// the rows copied at the picture's pitch and stride.  Plumbing, not a hot path.
extern "C" int himg_hip_decode_into_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, uint8_t *dst_data,
                                       const himg_hip_dst *dst, int x, int y, int *width, int *height, int *channels) {
  if (!ctx || !packed || !width || !height || !channels) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  if (int rc = himg_hip_peek(packed, packed_size, &W, &H, &C)) return fail(ctx, rc, "not a HIMG stream");
  *width = W; *height = H; *channels = C;
  if (!dst_data || !dst) return fail(ctx, HIMG_ERR_ARG, "bad argument");
  himg_hip_dst one = *dst;
  one.frame_pitch = 0;
  const int32_t org[2] = {x, y};
  size_t extent = 0;
  if (const char *bad = dst_check(&one, C, 1, org, W, H, &extent)) return fail(ctx, HIMG_ERR_ARG, bad);
  if (int rc = decode_core(ctx, packed, packed_size, &W, &H, &C)) return rc;
  std::vector<uint8_t> pix(ctx->host_bytes);
  HIP_TRY(ctx, hipMemcpy(pix.data(), ctx->h_out.p, pix.size(), hipMemcpyDeviceToHost));
  const size_t ps = (size_t)one.pixel_stride;
  for (int i = 0; i < H; ++i) {
    const uint8_t *srow = pix.data() + (size_t)i * W * C;
    uint8_t *drow = dst_data + (size_t)(y + i) * one.row_pitch + (size_t)x * ps;
    if (ps == (size_t)C) memcpy(drow, srow, (size_t)W * C);
    else
      for (int j = 0; j < W; ++j) memcpy(drow + (size_t)j * ps, srow + (size_t)j * C, (size_t)C);
  }
  return HIMG_OK;
}

// ---- batched host API: frames in flight ------------------------------------------

static int pipe_init(himg_hip_ctx *ctx) {
  himg_hip_ctx::Pipe &p = ctx->pipe;
  if (p.ready) return HIMG_OK;
  HIP_TRY(ctx, hipStreamCreateWithFlags(&p.s_in, hipStreamNonBlocking));
  HIP_TRY(ctx, hipStreamCreateWithFlags(&p.s_comp, hipStreamNonBlocking));
  HIP_TRY(ctx, hipStreamCreateWithFlags(&p.s_out, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(ctx, hipEventCreateWithFlags(&p.ev_in[k], hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&p.ev_k[k], hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&p.ev_out[k], hipEventDisableTiming));
    if (!p.meta[k].reserve(256)) return fail(ctx, HIMG_ERR_HIP, "staging allocation failed");
  }
  HIP_TRY(ctx, hipHostMalloc((void **)&p.h_meta, sizeof(PipeMeta), hipHostMallocDefault));
  p.ready = true;
  return HIMG_OK;
}

// The slot's HostResult on its way to its pinned mirror, behind the slot's kernels.
static int pipe_fetch_result(himg_hip_ctx *ctx, int slot) {
  himg_hip_ctx::Pipe &p = ctx->pipe;
  HIP_TRY(ctx, hipMemcpyAsync(&p.h_meta->res[slot], p.meta[slot].p, sizeof(HostResult), hipMemcpyDeviceToHost, p.s_comp));
  HIP_TRY(ctx, hipEventRecord(p.ev_k[slot], p.s_comp));
  return HIMG_OK;
}

// The three batch forms of the host encode (rq: frame i's budget / target at [i], its results to [i]).
static int encode_batch(himg_hip_ctx *ctx, const uint8_t *const *frames, int n, int width,
                        int height, int pixel_stride, int num_channels,
                        int use_ycbcr, const HostEncReq &rq, uint8_t *const *dst, const size_t *dst_cap,
                        size_t *out_sizes) {
  if (!ctx || !frames || !dst || !dst_cap || !out_sizes || n < 0) return HIMG_ERR_ARG;
  if (rq.kind != kEncPlain && !req_range_ok(ctx, rq)) return HIMG_ERR_ARG;
  Geom g;
  if (!make_geom(width, height, pixel_stride, num_channels, use_ycbcr, &g))
    return fail(ctx, HIMG_ERR_ARG, "bad geometry");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = pipe_init(ctx);
  if (rc) return rc;
  himg_hip_ctx::Pipe &p = ctx->pipe;
  const size_t cap = himg_hip_max_packed_size(width, height, num_channels);
  for (int k = 0; k < 2; ++k)
    if (!p.in[k].reserve(round_up((size_t)g.frame_bytes, 256)) || !p.out[k].reserve(cap))
      return fail(ctx, HIMG_ERR_HIP, "staging allocation failed");
  ctx->host_bytes = 0;
  int first_err = HIMG_OK;
  // Fetch frame j's verdict and start the copy of its stream.
  auto finish = [&](int j) -> int {
    const int slot = j & 1;
    out_sizes[j] = 0;
    HIP_TRY(ctx, hipEventSynchronize(p.ev_k[slot]));
    const HostResult r = p.h_meta->res[slot];
    int err = encode_verdict(ctx, rq, j, r);
    if (!err && (!dst[j] || dst_cap[j] < r.size)) err = fail(ctx, HIMG_ERR_CAPACITY, "output buffer too small");
    if (!err) {
      HIP_TRY(ctx, hipMemcpyAsync(dst[j], p.out[slot].p, r.size, hipMemcpyDeviceToHost, p.s_out));
      out_sizes[j] = r.size;
    } else if (!first_err) {
      first_err = err;
    }
    HIP_TRY(ctx, hipEventRecord(p.ev_out[slot], p.s_out));
    return HIMG_OK;
  };
  for (int i = 0; i < n; ++i) {
    const int slot = i & 1;
    if (!frames[i]) return fail(ctx, HIMG_ERR_ARG, "null frame");
    if (i >= 2) HIP_TRY(ctx, hipEventSynchronize(p.ev_out[slot]));   // staging of frame i-2 is free again
    HIP_TRY(ctx, hipMemcpyAsync(p.in[slot].p, frames[i], (size_t)g.frame_bytes, hipMemcpyHostToDevice, p.s_in));
    HIP_TRY(ctx, hipEventRecord(p.ev_in[slot], p.s_in));
    HIP_TRY(ctx, hipStreamWaitEvent(p.s_comp, p.ev_in[slot], 0));
    rc = encode_request_device(ctx, rq, i, p.in[slot].p, width, height, pixel_stride, num_channels, use_ycbcr,
                               p.out[slot].p, cap, (HostResult *)p.meta[slot].p, p.s_comp);
    if (rc) return rc;
    if ((rc = pipe_fetch_result(ctx, slot))) return rc;
    if (i >= 1 && (rc = finish(i - 1))) return rc;
  }
  if (n >= 1 && (rc = finish(n - 1))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(p.s_out));
  return first_err;
}

extern "C" int himg_hip_encode_batch(himg_hip_ctx *ctx, const uint8_t *const *frames, int n, int width,
                                     int height, int pixel_stride, int num_channels, int quality,
                                     int use_ycbcr, uint8_t *const *dst, const size_t *dst_cap,
                                     size_t *out_sizes) {
  const HostEncReq rq = {kEncPlain, quality};
  return encode_batch(ctx, frames, n, width, height, pixel_stride, num_channels, use_ycbcr, rq, dst, dst_cap, out_sizes);
}

extern "C" int himg_hip_encode_budget_batch(himg_hip_ctx *ctx, const uint8_t *const *frames, int n, int width,
                                            int height, int pixel_stride, int num_channels, int qmin, int qmax,
                                            int use_ycbcr, const size_t *budgets, uint8_t *const *dst,
                                            const size_t *dst_cap, size_t *out_sizes, int *qualities) {
  if (!ctx || !budgets || !qualities || n < 0) return HIMG_ERR_ARG;
  for (int i = 0; i < n; ++i) qualities[i] = -1;
  const HostEncReq rq = {kEncBudget, 0, qmin, qmax, budgets, nullptr, qualities, nullptr};
  return encode_batch(ctx, frames, n, width, height, pixel_stride, num_channels, use_ycbcr, rq, dst, dst_cap, out_sizes);
}

extern "C" int himg_hip_encode_target_batch(himg_hip_ctx *ctx, const uint8_t *const *frames, int n, int width,
                                            int height, int pixel_stride, int num_channels, int qmin, int qmax,
                                            int use_ycbcr, const uint64_t *max_sse, uint8_t *const *dst,
                                            const size_t *dst_cap, size_t *out_sizes, int *qualities, uint64_t *sses) {
  if (!ctx || !max_sse || !qualities || !sses || n < 0) return HIMG_ERR_ARG;
  for (int i = 0; i < n; ++i) { qualities[i] = -1; sses[i] = 0; }
  const HostEncReq rq = {kEncTarget, 0, qmin, qmax, nullptr, max_sse, qualities, sses};
  return encode_batch(ctx, frames, n, width, height, pixel_stride, num_channels, use_ycbcr, rq, dst, dst_cap, out_sizes);
}

extern "C" int himg_hip_decode_batch(himg_hip_ctx *ctx, const uint8_t *const *packed,
                                     const size_t *packed_sizes, int n, uint8_t *const *dst,
                                     const size_t *dst_cap, int *widths, int *heights, int *channels) {
  if (!ctx || !packed || !packed_sizes || !dst || !dst_cap || !widths || !heights || !channels || n < 0)
    return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = pipe_init(ctx);
  if (rc) return rc;
  himg_hip_ctx::Pipe &p = ctx->pipe;
  ctx->host_bytes = 0;
  int first_err = HIMG_OK;
  std::vector<size_t> out_bytes((size_t)n, 0);
  std::vector<int> launched((size_t)n, 0);
  auto finish = [&](int j) -> int {
    const int slot = j & 1;
    if (launched[j]) {
      HIP_TRY(ctx, hipEventSynchronize(p.ev_k[slot]));
      const int32_t st = p.h_meta->res[slot].status;
      const Piece pc = {0, out_bytes[j], dst[j], dst_cap[j]};
      const int err = st ? status_error(ctx, st) : pieces_fit(ctx, &pc, 1);
      if (!err) HIP_TRY(ctx, hipMemcpyAsync(dst[j], p.out[slot].p, out_bytes[j], hipMemcpyDeviceToHost, p.s_out));
      else { widths[j] = heights[j] = channels[j] = 0; if (!first_err) first_err = err; }
    }
    HIP_TRY(ctx, hipEventRecord(p.ev_out[slot], p.s_out));
    return HIMG_OK;
  };
  for (int i = 0; i < n; ++i) {
    const int slot = i & 1;
    widths[i] = heights[i] = channels[i] = 0;
    if (i >= 2) HIP_TRY(ctx, hipEventSynchronize(p.ev_out[slot]));
    int W = 0, H = 0, C = 0;
    Geom g;
    const char *msg = packed[i] ? parse_header(packed[i], packed_sizes[i], &W, &H, &C) : "Not a RIFF HIMG file.\n";
    if (msg || !make_geom(W, H, C, C, 1, &g)) {
      if (!first_err) first_err = msg ? fail(ctx, HIMG_ERR_FORMAT, msg) : fail(ctx, HIMG_ERR_UNSUPPORTED, "unsupported geometry");
    } else {
      const size_t in_cap = stage_slot(packed_sizes[i]);
      out_bytes[i] = (size_t)W * H * C;
      if (!p.in[slot].reserve(in_cap) || !p.out[slot].reserve(round_up(out_bytes[i], 256)))
        return fail(ctx, HIMG_ERR_HIP, "staging allocation failed");
      HIP_TRY(ctx, hipMemcpyAsync(p.in[slot].p, packed[i], packed_sizes[i], hipMemcpyHostToDevice, p.s_in));
      HIP_TRY(ctx, hipEventRecord(p.ev_in[slot], p.s_in));
      HIP_TRY(ctx, hipStreamWaitEvent(p.s_comp, p.ev_in[slot], 0));
      p.h_meta->dec_size[slot] = (uint32_t)packed_sizes[i];   // pinned: stays valid until the copy has run
      rc = himg_hip_decode_device(ctx, p.in[slot].p, in_cap, &p.h_meta->dec_size[slot], 1, W, H, C, p.out[slot].p,
                                  &((HostResult *)p.meta[slot].p)->status, p.s_comp);
      if (rc) return rc;
      if ((rc = pipe_fetch_result(ctx, slot))) return rc;
      widths[i] = W; heights[i] = H; channels[i] = C;
      launched[i] = 1;
    }
    if (i >= 1 && (rc = finish(i - 1))) return rc;
  }
  if (n >= 1 && (rc = finish(n - 1))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(p.s_out));
  return first_err;
}

// ---------------------------------------------------------------------------
// 1/8-scale preview: the LRES chunk's plane as a picture (kernels_dec.hip, launch_preview).
// ---------------------------------------------------------------------------
// The reference's first four stages on the host, headers only (decoder.cpp:144-212,428-461):
// RIFF, FRMT, the LMAP body (mapper.cpp:127-157, with the engine's size limit of k_dec_parse),
// and the forward search for LRES.  Nothing at or beyond `avail` is read.  Returns HIMG_OK with
// *head = the end of the LRES chunk, HIMG_ERR_FORMAT (and the reference's message for the stage)
// where the reference rejects the head, HIMG_ERR_CAPACITY where `avail` ends first (*head set
// when the LRES header was reached), HIMG_ERR_UNSUPPORTED for a geometry beyond the engine's.
static int preview_walk(const uint8_t *p, size_t avail, size_t packed_size, int *W, int *H, int *C, size_t *head,
                        const char **msg) {
  static const char *kMsg[] = {"Not a RIFF HIMG file.\n", "Error decoding header.\n",
                               "Error decoding low-res mapping function.\n", "Error decoding low-res data.\n"};
  *head = 0;
  *msg = nullptr;
  if (packed_size < 12 || packed_size > 0x7fffffffu) return *msg = kMsg[0], HIMG_ERR_FORMAT;
  if (avail < 12) return HIMG_ERR_CAPACITY;
  uint32_t riff;
  memcpy(&riff, p + 4, 4);
  if (memcmp(p, "RIFF", 4) != 0 || (size_t)riff + 8 != packed_size || memcmp(p + 8, "HIMG", 4) != 0)
    return *msg = kMsg[0], HIMG_ERR_FORMAT;
  static const char *kTag[3] = {"FRMT", "LMAP", "LRES"};
  size_t idx = 12;
  for (int t = 0; t < 3; ++t) {
    uint32_t sz = 0;
    for (;;) {   // host_find_chunk, with the bytes present checked first
      if (idx + 8 > packed_size) return *msg = kMsg[t + 1], HIMG_ERR_FORMAT;
      if (idx + 8 > avail) return HIMG_ERR_CAPACITY;
      memcpy(&sz, p + idx + 4, 4);
      const bool hit = memcmp(p + idx, kTag[t], 4) == 0;
      idx += 8;
      if (sz > 0x7fffffffu || idx + sz > packed_size) return *msg = kMsg[t + 1], HIMG_ERR_FORMAT;
      if (hit) break;
      idx += sz;
    }
    if (t == 2) {
      *head = idx + sz;
      return idx + sz > avail ? HIMG_ERR_CAPACITY : HIMG_OK;
    }
    if (idx + sz > avail) return HIMG_ERR_CAPACITY;
    const uint8_t *b = p + idx;
    if (t == 0) {
      if (sz < 11 || b[0] != 1) return *msg = kMsg[1], HIMG_ERR_FORMAT;
      uint32_t w, h;
      memcpy(&w, b + 1, 4);
      memcpy(&h, b + 5, 4);
      *W = (int)w; *H = (int)h; *C = b[9];
      Geom g;
      if (!make_geom(*W, *H, *C, *C, 1, &g)) return HIMG_ERR_UNSUPPORTED;
    } else if (!(sz >= 1 && sz <= (uint32_t)kTreeStride && b[0] <= 127 && 1u + b[0] + 2u * (127u - b[0]) == sz)) {
      return *msg = kMsg[2], HIMG_ERR_FORMAT;
    }
    idx += sz;
  }
  return HIMG_ERR_FORMAT;   // (not reached)
}

extern "C" int himg_hip_preview_peek(const uint8_t *packed, size_t avail, size_t packed_size, int *pw, int *ph,
                                     int *channels, size_t *head_bytes) {
  if (!packed || !pw || !ph || !channels || !head_bytes) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  size_t head = 0;
  const char *msg = nullptr;
  const int rc = preview_walk(packed, avail, packed_size, &W, &H, &C, &head, &msg);
  *head_bytes = head;
  if (rc == HIMG_OK) { *pw = (W + 7) / 8; *ph = (H + 7) / 8; *channels = C; }
  return rc;
}

// The device launch behind every preview entry point; d_packed holds the streams at in_stride,
// each readable up to its head rounded up to 4 bytes.
static int preview_launch(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_sizes,
                          int batch, int width, int height, int num_channels, void *d_out, int32_t *d_status,
                          void *stream) {
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, batch, kWsHead, d_packed, d_out, &in_stride, nullptr, &g))
    return rc;
  if (int rc = decode_begin(ctx, g, batch, kWsHead, h_sizes, stream, &d_sizes)) return rc;
  launch_preview(g, ctx->dec_ws, batch, (const uint8_t *)d_packed, in_stride, d_sizes, (uint32_t *)ctx->d_sizes.p + batch,
                 (uint8_t *)d_out, d_status, (hipStream_t)stream, &ctx->prof);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_preview_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                       const uint32_t *h_sizes, int batch, int width, int height, int num_channels,
                                       void *d_out, int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_out || !d_status || batch < 1 || batch > 65535) return HIMG_ERR_ARG;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  return preview_launch(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, d_out, d_status, stream);
}

// ---------------------------------------------------------------------------
// Decode of a stream prefix: whole block rows exact, the rest from the low-res plane
// (kernels_dec.hip, launch_prefix; the walk's rules: prefix_walk.h, shared with the device).
// ---------------------------------------------------------------------------
static const char kPrefixShort[] = "the prefix ends before the first block row";
static const char kPrefixState[] = "the state does not belong to this prefix";
static uint32_t prefix_avail32(size_t avail) { return avail > 0x80000000u ? 0x80000000u : (uint32_t)avail; }

static_assert(sizeof(himg_hip_prefix_state) == 16 && sizeof(himg_dev::PfxState) == 16, "the state is four words");

// himg_hip_prefix_peek; `state` given and started: the row walk resumes there (himg_hip_prefix_peek_from).
static int prefix_peek_impl(const uint8_t *packed, size_t avail, int fix_t2, const himg_hip_prefix_state *state,
                            himg_hip_prefix_plan *plan) {
  *plan = himg_hip_prefix_plan();
  const uint32_t av = prefix_avail32(avail);
  const bool resume = state && state->started;
  if (resume && av < state->avail_seen) return HIMG_ERR_ARG;
  himg_dev::PfxHead h;
  int rc = himg_dev::pfx_chain(packed, av, fix_t2, 0, &h);
  plan->packed_size = h.T;
  if (h.frmt) {   // FRMT was reached: its fields are untrusted (himg_hip_peek)
    Geom g;
    if (!make_geom((int)h.W, (int)h.H, (int)h.C, (int)h.C, 1, &g)) return HIMG_ERR_UNSUPPORTED;
    plan->width = (int)h.W; plan->height = (int)h.H; plan->num_channels = (int)h.C;
    plan->rows = g.rows;
  }
  if (rc == himg_dev::kPfxFormat) return h.need > av ? HIMG_ERR_CAPACITY : HIMG_ERR_FORMAT;
  if (rc == himg_dev::kPfxShort) return HIMG_ERR_CAPACITY;
  const uint32_t cnt = h.csz < (uint32_t)kTreeStride ? h.csz : (uint32_t)kTreeStride;
  const uint32_t have = av > h.coff ? (av - h.coff < cnt ? av - h.coff : cnt) : 0u;
  uint32_t tb = 0;
  rc = himg_dev::pfx_tree_len(packed + h.coff, have, h.csz, &tb);
  if (rc == himg_dev::kPfxFormat) return HIMG_ERR_FORMAT;
  const uint32_t q = h.coff + tb, end = h.coff + h.csz;
  if (tb) {
    if (q >= end) return HIMG_ERR_FORMAT;   // nothing behind the tree (huffman_dec.cpp:277-278)
    plan->head_bytes = q;
  }
  if (rc == himg_dev::kPfxShort) return HIMG_ERR_CAPACITY;
  himg_dev::PfxRows pr;
  if (resume) {
    const himg_dev::PfxState s = {state->started, state->rows_done, state->walk_pos, state->avail_seen};
    if (!himg_dev::pfx_state_ok(s, av, plan->rows, q, end)) return *plan = himg_hip_prefix_plan(), HIMG_ERR_ARG;
    rc = himg_dev::pfx_rows_from(packed, av, h.T, fix_t2, plan->rows, s.walk_pos, s.rows_done, end, nullptr, nullptr, &pr);
  } else {
    rc = himg_dev::pfx_rows(packed, av, h.T, fix_t2, plan->rows, q, end, nullptr, nullptr, &pr);
  }
  if (rc != himg_dev::kPfxOk) return HIMG_ERR_FORMAT;
  plan->rows_complete = pr.k;
  plan->used_bytes = pr.used;
  plan->next_bytes = pr.next;
  return HIMG_OK;
}

extern "C" int himg_hip_prefix_peek(const uint8_t *packed, size_t avail, int fix_t2, himg_hip_prefix_plan *plan) {
  if (!plan || (!packed && avail)) return HIMG_ERR_ARG;
  return prefix_peek_impl(packed, avail, fix_t2, nullptr, plan);
}

extern "C" int himg_hip_prefix_peek_from(const uint8_t *packed, size_t avail, int fix_t2,
                                         const himg_hip_prefix_state *state, himg_hip_prefix_plan *plan) {
  if (!plan || !state || (!packed && avail)) return HIMG_ERR_ARG;
  return prefix_peek_impl(packed, avail, fix_t2, state, plan);
}

// What the two device entry points of the prefix decode run behind their argument checks.  d_state: the
// continued decode's states, or nullptr (kernels_dec.hip, launch_prefix).
static int prefix_launch(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_avail, int batch,
                         int width, int height, int num_channels, himg_hip_prefix_state *d_state, void *d_out,
                         int32_t *d_rows, int32_t *d_status, void *stream) {
  if (int rc = stride_covers(ctx, h_avail, batch, in_stride)) return rc;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, batch, kWsRegion, d_packed, d_out, &in_stride, nullptr, &g))
    return rc;
  // (the bytes present ride to the device as the packed sizes do: no wait; seven more words per frame
  // behind them are the walk's, himg_dev::launch_prefix)
  if (int rc = decode_begin(ctx, g, batch, kWsRegion, h_avail, stream, &d_sizes)) return rc;
  launch_prefix(g, ctx->dec_ws, batch, (const uint8_t *)d_packed, in_stride, (uint32_t *)ctx->d_sizes.p,
                (himg_dev::PfxState *)d_state, (uint8_t *)d_out, d_rows, d_status, (hipStream_t)stream, &ctx->prof,
                ctx->opts.use_side ? &ctx->dstr : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_prefix_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                             const uint32_t *h_avail, int batch, int width, int height,
                                             int num_channels, void *d_out, int32_t *d_rows, int32_t *d_status,
                                             void *stream) {
  if (!ctx || !d_packed || !h_avail || !d_out || !d_rows || !d_status || batch < 1 || batch > 65535) return HIMG_ERR_ARG;
  return prefix_launch(ctx, d_packed, in_stride, h_avail, batch, width, height, num_channels, nullptr, d_out, d_rows,
                       d_status, stream);
}

extern "C" int himg_hip_decode_prefix_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t avail, uint8_t *dst,
                                         size_t dst_cap, int *width, int *height, int *channels, int *rows_complete) {
  if (!ctx || (!packed && avail) || !width || !height || !channels || !rows_complete) return HIMG_ERR_ARG;
  *rows_complete = -1;
  // The host needs the geometry alone, to size the launch: the chunk headers as far as FRMT.  Every
  // check is the device's (k_span_gate, k_dec_parse_prefix), which words the verdict.
  const uint32_t av = prefix_avail32(avail);
  himg_dev::PfxHead h;
  const int hc = himg_dev::pfx_chain(packed, av, ctx->fix_t2, 0, &h);
  if (!h.frmt) {
    if (hc == himg_dev::kPfxShort) return fail(ctx, HIMG_ERR_CAPACITY, kPrefixShort);
    return fail(ctx, HIMG_ERR_FORMAT, h.stage == 1 ? "Not a RIFF HIMG file.\n" : "Error decoding header.\n");
  }
  const int W = (int)h.W, H = (int)h.H, C = (int)h.C;
  Geom g;
  if (!make_geom(W, H, C, C, 1, &g)) return fail(ctx, HIMG_ERR_UNSUPPORTED, "unsupported geometry");
  const size_t out_bytes = (size_t)W * H * C;
  if (int rc = stage_whole(ctx, packed, av, out_bytes, 8)) return rc;   // (only the bytes present)
  int32_t *d_st = (int32_t *)ctx->h_status.p;   // the status word, then k
  int rc = himg_hip_decode_prefix_device(ctx, ctx->h_in.p, stage_slot(av), &av, 1, W, H, C, ctx->h_out.p, d_st + 1, d_st,
                                         nullptr);
  int32_t st[2] = {0, -1};
  if ((rc = stage_verdict(ctx, rc, st, 2, kPrefixShort))) return rc;
  *rows_complete = st[1];
  const Piece pc = {0, out_bytes, dst, dst_cap};
  return deliver(ctx, W, H, C, width, height, channels, out_bytes, &pc, 1);
}

// The prefix decode continued from the rows a caller's picture already holds (kernels_dec.hip,
// launch_prefix with states): the states are read, judged and advanced on the device.
extern "C" int himg_hip_decode_prefix_more_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                                  const uint32_t *h_avail, int batch, int width, int height,
                                                  int num_channels, himg_hip_prefix_state *d_state, void *d_out,
                                                  int32_t *d_rows, int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_avail || !d_state || !d_out || !d_rows || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  if ((uintptr_t)d_state & 15) return fail(ctx, HIMG_ERR_ARG, "the states must be 16-byte aligned");
  return prefix_launch(ctx, d_packed, in_stride, h_avail, batch, width, height, num_channels, d_state, d_out, d_rows,
                       d_status, stream);
}

extern "C" int himg_hip_decode_prefix_more_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t avail,
                                              himg_hip_prefix_state *state, uint8_t *dst, size_t dst_cap, int *width,
                                              int *height, int *channels, int *rows_complete) {
  if (!ctx || (!packed && avail) || !state || !width || !height || !channels || !rows_complete) return HIMG_ERR_ARG;
  *rows_complete = -1;
  // The host's own walk says what to upload; every verdict on the stream is the device's (decode_prefix_to).
  const uint32_t av = prefix_avail32(avail);
  himg_hip_prefix_plan plan;
  const int pc = prefix_peek_impl(packed, av, ctx->fix_t2, state, &plan);
  if (pc == HIMG_ERR_ARG) return fail(ctx, HIMG_ERR_ARG, kPrefixState);
  if (pc == HIMG_ERR_UNSUPPORTED) return fail(ctx, HIMG_ERR_UNSUPPORTED, "unsupported geometry");
  if (!plan.num_channels) {   // FRMT has not arrived, or the walk failed before it
    if (pc == HIMG_ERR_CAPACITY) return fail(ctx, HIMG_ERR_CAPACITY, kPrefixShort);
    return fail(ctx, HIMG_ERR_FORMAT, plan.packed_size ? "Error decoding header.\n" : "Not a RIFF HIMG file.\n");
  }
  const int W = plan.width, H = plan.height, C = plan.num_channels;
  const size_t row_bytes = (size_t)W * C, out_bytes = (size_t)H * row_bytes;
  const Piece whole = {0, out_bytes, dst, dst_cap};
  if (int rc = out_check(ctx, W, H, C, width, height, channels, &whole, 1)) return rc;
  const size_t in_cap = stage_slot(av);
  // A resumed state the host's walk accepts: the head and the bytes from the walk's position on, each at its
  // offset (the bytes between them are the rows already decoded: nothing reads them).  Else the whole prefix.
  // h_status: the status word, k, then the state at byte 16.  (Nothing stays resident: no fetch_last behind
  // this call.)
  const bool partial = state->started && pc == HIMG_OK;
  const size_t ranges[4] = {0, plan.head_bytes, state->walk_pos, av};
  if (int rc = stage_reserve(ctx, ctx->h_in, in_cap, out_bytes, 32, 0)) return rc;
  uint8_t *d_in = (uint8_t *)ctx->h_in.p;
  if (int rc = stage_upload(ctx, d_in, in_cap, packed, av, partial ? ranges : nullptr, partial ? 2 : 0)) return rc;
  int32_t *d_st = (int32_t *)ctx->h_status.p;
  himg_hip_prefix_state *d_state = (himg_hip_prefix_state *)((uint8_t *)ctx->h_status.p + 16);
  HIP_TRY(ctx, hipMemcpyAsync(d_state, state, sizeof(*state), hipMemcpyHostToDevice, nullptr));
  int rc = himg_hip_decode_prefix_more_device(ctx, d_in, in_cap, &av, 1, W, H, C, d_state, ctx->h_out.p, d_st + 1, d_st,
                                              nullptr);
  struct { int32_t st, k, pad[2]; himg_hip_prefix_state s; } back;
  if ((rc = stage_verdict(ctx, rc, &back.st, sizeof(back) / 4, kPrefixShort, nullptr, kPrefixState))) return rc;
  // A fresh state: the whole picture; else the pixel rows of block rows [k_prev, k_new) alone.
  const size_t y0 = state->started ? 8 * (size_t)state->rows_done : 0;
  const size_t y1 = state->started ? (8 * (size_t)back.k < (size_t)H ? 8 * (size_t)back.k : (size_t)H) : (size_t)H;
  const Piece rows = {y0 * row_bytes, y1 > y0 ? (y1 - y0) * row_bytes : 0, dst + y0 * row_bytes, dst_cap};
  if ((rc = pieces_copy(ctx, &rows, 1))) return rc;
  *state = back.s;
  *rows_complete = back.k;
  return HIMG_OK;
}

// ---------------------------------------------------------------------------
// The concealing decode: the full decode, then the block rows it rejected -- or could not delimit -- from
// the low-res plane (kernels_dec.hip, launch_conceal).
// ---------------------------------------------------------------------------
extern "C" int himg_hip_decode_conceal_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                              const uint32_t *h_sizes, int batch, int width, int height,
                                              int num_channels, void *d_out, int32_t *d_concealed, uint8_t *d_rowmap,
                                              int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_out || !d_concealed || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, batch, kWsFull, d_packed, d_out, &in_stride, nullptr, &g))
    return rc;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  { uint32_t mx = 0; for (int i = 0; i < batch; ++i) mx = h_sizes[i] > mx ? h_sizes[i] : mx; g.wide_q = wide_q_hint(g, mx); }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->d_cmap.reserve(round_up((size_t)batch * g.rows, 256)))
    return fail(ctx, HIMG_ERR_HIP, "decoder workspace allocation failed");
  // (the sizes ride to the device as in decode_device: no wait; four more words per frame behind them
  // are the repair pass's, himg_dev::launch_conceal)
  if (int rc = decode_begin(ctx, g, batch, kWsFull, h_sizes, stream, &d_sizes)) return rc;
  launch_conceal(g, ctx->dec_ws, batch, (const uint8_t *)d_packed, in_stride, (uint32_t *)ctx->d_sizes.p,
                 (uint8_t *)ctx->d_cmap.p, (uint8_t *)d_out, d_concealed, d_rowmap, d_status, (hipStream_t)stream,
                 &ctx->prof, ctx->opts, ctx->opts.use_side ? &ctx->dstr : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_conceal_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, uint8_t *dst,
                                          size_t dst_cap, int *width, int *height, int *channels, uint8_t *rowmap,
                                          size_t rowmap_cap, int *concealed) {
  if (!ctx || !packed || !width || !height || !channels || !concealed) return HIMG_ERR_ARG;
  *concealed = -1;
  int W = 0, H = 0, C = 0;
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, &W, &H, &C, &g)) return rc;
  if (rowmap && rowmap_cap < (size_t)g.rows) return fail(ctx, HIMG_ERR_CAPACITY, "row map buffer too small");
  // The whole stream goes up and the device walks it: the host index cannot be built over a bad header.
  const size_t out_bytes = (size_t)W * H * C;
  const size_t map_at = 256;   // (h_status: the status word, the count, then the row map)
  if (int rc = stage_whole(ctx, packed, packed_size, out_bytes, map_at + (size_t)g.rows)) return rc;
  const uint32_t sz32 = (uint32_t)packed_size;
  int32_t *d_st = (int32_t *)ctx->h_status.p;
  uint8_t *d_map = (uint8_t *)ctx->h_status.p + map_at;
  int rc = himg_hip_decode_conceal_device(ctx, ctx->h_in.p, stage_slot(packed_size), &sz32, 1, W, H, C, ctx->h_out.p,
                                          d_st + 1, d_map, d_st, nullptr);
  int32_t st[2] = {0, -1};
  if ((rc = stage_verdict(ctx, rc, st, 2))) return rc;
  *concealed = st[1];
  if (rowmap) HIP_TRY(ctx, hipMemcpy(rowmap, d_map, (size_t)g.rows, hipMemcpyDeviceToHost));
  const Piece pc = {0, out_bytes, dst, dst_cap};
  return deliver(ctx, W, H, C, width, height, channels, out_bytes, &pc, 1);
}

// ---------------------------------------------------------------------------
// Region decode: one rectangle at full resolution (kernels_dec.hip, launch_region).
// ---------------------------------------------------------------------------
static bool region_ok(int W, int H, int x, int y, int w, int h) {
  return w >= 1 && h >= 1 && x >= 0 && y >= 0 && (long long)x + w <= W && (long long)y + h <= H;
}

// A rectangle R of the picture at scale 2^-sl (sl = 0: the full-resolution picture, sl = 1, 2: the
// scaled decode's, ceil(W / F) x ceil(H / F)): false when R does not lie inside it.  up[4]: the
// full-resolution rectangle R covers, (F x, F y, min(F w, W - F x), min(F h, H - F y)) -- the one
// whose block rows, verdict and bytes used are R's.
static bool rect_up(int W, int H, int sl, int x, int y, int w, int h, int up[4]) {
  const int F = 1 << sl;
  const int ow = (int)(((long long)W + F - 1) / F), oh = (int)(((long long)H + F - 1) / F);
  if (!region_ok(ow, oh, x, y, w, h)) return false;
  up[0] = F * x; up[1] = F * y;
  up[2] = (long long)F * w < W - up[0] ? F * w : W - up[0];
  up[3] = (long long)F * h < H - up[1] ? F * h : H - up[1];
  return true;
}

// The plan of rectangle (x, y, w, h): host_walk bounded at the rectangle's last block row.
static int region_index(const uint8_t *packed, size_t packed_size, int fix_t2, int x, int y, int w, int h,
                        himg_hip_region_plan *plan, uint32_t *row_index) {
  int W = 0, H = 0, C = 0;
  int rc = himg_hip_peek(packed, packed_size, &W, &H, &C);
  if (rc) return rc;
  plan->width = W; plan->height = H; plan->num_channels = C;
  if (!region_ok(W, H, x, y, w, h)) return HIMG_ERR_ARG;
  plan->row0 = y / 8; plan->row1 = (y + h + 7) / 8;
  return host_walk(packed, packed_size, fix_t2, (H + 7) / 8, plan->row0, plan->row1, plan, row_index);
}

extern "C" int himg_hip_region_peek(const uint8_t *packed, size_t packed_size, int fix_t2, int x, int y, int w, int h,
                                    himg_hip_region_plan *plan) {
  if (!packed || !plan) return HIMG_ERR_ARG;
  *plan = himg_hip_region_plan();
  return region_index(packed, packed_size, fix_t2, x, y, w, h, plan, nullptr);
}

// The device launch behind every region entry point: the window w x h at frame f's origin
// (h_org[2 f], h_org[2 f + 1]); every origin is checked before anything is launched.
// d_row_index: the host's index, 2 x rows words per frame (rows r0_f .. r1_f - 1 filled).
// scale_log2 = 1, 2: the window and the origins are those of the scaled picture (k_dec_scaled_region);
// what reaches the device are the origins of the full-resolution rectangles the windows cover.
// form (scale_log2 = 0 only): the caller's checked descriptor.  kStorePitch: d_out holds the destination
// pictures, frame f's window at h_dst_org[2 f], [2 f + 1], and bad_dst is what dst_check found wrong.
static int region_launch(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_sizes, int batch,
                         int width, int height, int num_channels, const int32_t *h_org, int w, int h,
                         const uint32_t *d_row_index, void *d_out, int32_t *d_status, void *stream, int scale_log2 = 0,
                         himg_dev::StoreForm form = himg_dev::StoreForm(), const int32_t *h_dst_org = nullptr,
                         const char *bad_dst = nullptr) {
  if (scale_log2 < 0 || scale_log2 > 2) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1 or 2");
  if (scale_log2 && form.kind != himg_dev::kStoreU8) return fail(ctx, HIMG_ERR_ARG, "a descriptor at full scale only");
  const bool pitch = form.kind == himg_dev::kStorePitch;
  std::vector<int32_t> up_org;
  if (scale_log2) up_org.resize(2 * (size_t)batch);
  const char *bad = nullptr;
  for (int f = 0; f < batch && !bad; ++f) {
    int up[4];
    if (!rect_up(width, height, scale_log2, h_org[2 * f], h_org[2 * f + 1], w, h, up)) bad = "bad rectangle";
    else if (scale_log2) { up_org[2 * f] = up[0]; up_org[2 * f + 1] = up[1]; }
  }
  if (scale_log2) h_org = up_org.data();
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, batch, kWsRegion, d_packed, d_out, &in_stride,
                           bad ? bad : bad_dst, &g))
    return rc;
  // (the origins ride with the sizes: no extra copy, no wait; the destinations' behind the windows')
  if (pitch) {
    up_org.assign(h_org, h_org + 2 * (size_t)batch);
    up_org.insert(up_org.end(), h_dst_org, h_dst_org + 2 * (size_t)batch);
    h_org = up_org.data();
  }
  if (int rc = decode_begin(ctx, g, batch, kWsRegion, h_sizes, stream, &d_sizes, h_org, pitch ? 2 : 1)) return rc;
  himg_dev::DstDesc dd;
  if (pitch) {
    dd = form.dst();
    dd.org = (const int32_t *)(d_sizes + 3 * (size_t)batch);
    form = &dd;
  }
  launch_region(g, ctx->dec_ws, batch, (const uint8_t *)d_packed, in_stride, d_sizes, d_row_index, h_org,
                (const int32_t *)(d_sizes + batch), scale_log2, w, h, (uint8_t *)d_out, d_status, (hipStream_t)stream,
                &ctx->prof, ctx->opts.use_side ? &ctx->dstr : nullptr, form);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_region_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                             const uint32_t *h_sizes, int batch, int width, int height,
                                             int num_channels, int x, int y, int w, int h, void *d_out,
                                             int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_out || !d_status || batch < 1 || batch > 65535) return HIMG_ERR_ARG;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  std::vector<int32_t> org(2 * (size_t)batch);
  for (int f = 0; f < batch; ++f) { org[2 * f] = x; org[2 * f + 1] = y; }
  return region_launch(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, org.data(), w, h, nullptr,
                       d_out, d_status, stream);
}

extern "C" int himg_hip_decode_regions_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                              const uint32_t *h_sizes, int batch, int width, int height,
                                              int num_channels, const int32_t *h_origins, int w, int h, void *d_out,
                                              int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !h_origins || !d_out || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  return region_launch(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, h_origins, w, h, nullptr,
                       d_out, d_status, stream);
}

// Many windows of one stream (kernels_dec.hip, launch_stream_regions): window k is the w x h rectangle at
// (h_org[2 k], h_org[2 k + 1]) of stream h_stream_of[k].  Every map entry and rectangle is checked before
// anything is launched.  The host holds every window, so it plans what the device shares between them: where
// each stream's walk stops, and the runs of block rows to count, each touched (stream, row) once.  All of it
// rides with the sizes in one pinned slot; the walk's and the windows' words follow it in d_sizes.
// d_row_index (one host stream, himg_hip_decode_stream_regions_to): the host's index of rows
// [index_rows[0], index_rows[1]).
static int stream_regions_launch(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_sizes,
                                 int n_streams, int width, int height, int num_channels, const int32_t *h_stream_of,
                                 const int32_t *h_org, int n_windows, int w, int h, const uint32_t *d_row_index,
                                 const int32_t *index_rows, void *d_out, int32_t *d_status, void *stream) {
  const char *bad = nullptr;
  for (int k = 0; k < n_windows && !bad; ++k) {
    if (h_stream_of[k] < 0 || h_stream_of[k] >= n_streams) bad = "stream_of outside the streams";
    else if (!region_ok(width, height, h_org[2 * k], h_org[2 * k + 1], w, h)) bad = "bad rectangle";
  }
  Geom g;
  if (!bad && height > 0 && num_channels > 0 && ((height + 7) / 8 + 1 > 65535 || (long long)n_streams * num_channels > 65535))
    bad = "grid too large";   // (HIMG_ERR_ARG here, like every other check of this entry)
  if (int rc = decode_args(ctx, width, height, num_channels, n_streams, kWsRegion, d_packed, d_out, &in_stride, bad, &g))
    return rc;
  // Each stream's touched rows: its windows' [r0_k, r1_k) sorted and merged.
  std::vector<std::vector<std::pair<int, int>>> runs(n_streams);
  for (int k = 0; k < n_windows; ++k)
    runs[h_stream_of[k]].push_back({h_org[2 * k + 1] / 8, (h_org[2 * k + 1] + h + 7) / 8});
  long long list_rows = 0;
  std::vector<int32_t> row_end(n_streams, 0);
  for (int s = 0; s < n_streams; ++s) {
    auto &v = runs[s];
    if (v.empty()) continue;
    std::sort(v.begin(), v.end());
    size_t m = 0;
    for (size_t i = 1; i < v.size(); ++i) {
      if (v[i].first <= v[m].second) v[m].second = v[i].second > v[m].second ? v[i].second : v[m].second;
      else v[++m] = v[i];
    }
    v.resize(m + 1);
    for (const auto &r : v) list_rows += r.second - r.first;
    row_end[s] = v.back().second == g.rows ? 0x7fffffff : v.back().second;
  }
  const int chunk = himg_dev::stream_count_chunk(g, list_rows);
  // The words: sizes, stream_of, origins, row_end, index_rows, then the count list.
  const size_t o_map = (size_t)n_streams, o_org = o_map + n_windows, o_end = o_org + 2 * (size_t)n_windows,
               o_idx = o_end + n_streams, o_list = o_idx + 2 * (size_t)n_streams;
  std::vector<uint32_t> words(o_list);
  memcpy(words.data(), h_sizes, (size_t)n_streams * 4);
  memcpy(words.data() + o_map, h_stream_of, (size_t)n_windows * 4);
  memcpy(words.data() + o_org, h_org, (size_t)n_windows * 8);
  memcpy(words.data() + o_end, row_end.data(), (size_t)n_streams * 4);
  for (int s = 0; s < n_streams; ++s) {
    words[o_idx + 2 * s] = index_rows ? (uint32_t)index_rows[2 * s] : 0u;
    words[o_idx + 2 * s + 1] = index_rows ? (uint32_t)index_rows[2 * s + 1] : 0u;
  }
  for (int s = 0; s < n_streams; ++s)
    for (const auto &r : runs[s])
      for (int a = r.first; a < r.second; a += chunk) {
        words.push_back((uint32_t)s); words.push_back((uint32_t)a);
        words.push_back((uint32_t)(a + chunk < r.second ? a + chunk : r.second));
      }
  const size_t n_list = (words.size() - o_list) / 3, n_scratch = 2 * (size_t)n_streams + n_windows;
  if (n_list > 0x7fffffffu) return fail(ctx, HIMG_ERR_UNSUPPORTED, "grid too large");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->d_sizes.reserve((words.size() + n_scratch) * 4)) return fail(ctx, HIMG_ERR_HIP, "decoder workspace allocation failed");
  if (int rc = ensure_dec_ws(ctx, g, n_streams, kWsRegion)) return rc;
  ctx->last_stream = (hipStream_t)stream;
  if (int rc = stage_words(ctx, ctx->d_sizes.p, words.data(), words.size(), nullptr, 0, ctx->last_stream)) return rc;
  const uint32_t *d_sizes = (const uint32_t *)ctx->d_sizes.p;
  const int32_t *dw = (const int32_t *)d_sizes;
  const himg_dev::StreamRegionWords sw = {dw + o_map, dw + o_org, dw + o_end, dw + o_list, dw + o_idx,
                                          (int32_t *)ctx->d_sizes.p + words.size()};
  himg_dev::launch_stream_regions(g, ctx->dec_ws, n_streams, (const uint8_t *)d_packed, in_stride, d_sizes, d_row_index, sw,
                                  n_windows, h_org, (int)n_list, list_rows, w, h, (uint8_t *)d_out, d_status,
                                  (hipStream_t)stream, &ctx->prof, ctx->opts.use_side ? &ctx->dstr : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_stream_regions_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                                     const uint32_t *h_sizes, int n_streams, int width, int height,
                                                     int num_channels, const int32_t *h_stream_of,
                                                     const int32_t *h_origins, int n_windows, int w, int h, void *d_out,
                                                     int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !h_stream_of || !h_origins || !d_out || !d_status || n_streams < 1 ||
      n_streams > 65535 || n_windows < 1 || n_windows > 65535)
    return HIMG_ERR_ARG;
  if (int rc = stride_covers(ctx, h_sizes, n_streams, in_stride)) return rc;
  return stream_regions_launch(ctx, d_packed, in_stride, h_sizes, n_streams, width, height, num_channels, h_stream_of,
                               h_origins, n_windows, w, h, nullptr, nullptr, d_out, d_status, stream);
}

extern "C" int himg_hip_decode_regions_tensor_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                                     const uint32_t *h_sizes, int batch, int width, int height,
                                                     int num_channels, const int32_t *h_origins, int w, int h,
                                                     const himg_hip_tensor_desc *t, void *d_out,
                                                     int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !h_origins || !t || !d_out || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  himg_dev::TensDesc td;
  if (!tensor_desc_ok(t, num_channels, &td)) return fail(ctx, HIMG_ERR_ARG, "bad tensor descriptor");
  return region_launch(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, h_origins, w, h, nullptr,
                       d_out, d_status, stream, 0, &td);
}

extern "C" int himg_hip_decode_regions_into_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                                   const uint32_t *h_sizes, int batch, int width, int height,
                                                   int num_channels, const int32_t *h_src_origins, int w, int h,
                                                   void *d_dst, const himg_hip_dst *dst, const int32_t *h_dst_origins,
                                                   int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !h_src_origins || !d_dst || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  if (!dst || !h_dst_origins) return fail(ctx, HIMG_ERR_ARG, "bad argument");
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  himg_dev::DstDesc dd;
  size_t extent = 0;
  const char *bad_dst = dst_check(dst, num_channels, batch, h_dst_origins, w, h, &extent, &dd);
  return region_launch(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, h_src_origins, w, h, nullptr,
                       d_dst, d_status, stream, 0, &dd, h_dst_origins, bad_dst);
}

// The scaled region decode's device entry: a window of the picture at 1/2 or 1/4 scale.  A rectangle of
// the scaled picture is planned, walked, counted and judged as the full-resolution rectangle it covers
// (rect_up); the entries are the region decode's with a scale.
extern "C" int himg_hip_decode_scaled_regions_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                                     const uint32_t *h_sizes, int batch, int width, int height,
                                                     int num_channels, int scale_log2, const int32_t *h_origins,
                                                     int w, int h, void *d_out, int32_t *d_status, void *stream) {
  if (!ctx || !d_packed || !h_sizes || !h_origins || !d_out || !d_status || batch < 1 || batch > 65535)
    return HIMG_ERR_ARG;
  if (scale_log2 != 1 && scale_log2 != 2) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1 or 2");
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  return region_launch(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, h_origins, w, h, nullptr,
                       d_out, d_status, stream, scale_log2);
}

extern "C" int himg_hip_scaled_region_peek(const uint8_t *packed, size_t packed_size, int fix_t2, int scale_log2, int x,
                                           int y, int w, int h, himg_hip_region_plan *plan) {
  if (!packed || !plan || (scale_log2 != 1 && scale_log2 != 2)) return HIMG_ERR_ARG;
  *plan = himg_hip_region_plan();
  int W = 0, H = 0, C = 0, up[4];
  if (int rc = himg_hip_peek(packed, packed_size, &W, &H, &C)) return rc;
  plan->width = W; plan->height = H; plan->num_channels = C;
  if (!rect_up(W, H, scale_log2, x, y, w, h, up)) return HIMG_ERR_ARG;
  return region_index(packed, packed_size, fix_t2, up[0], up[1], up[2], up[3], plan, nullptr);
}

// ---------------------------------------------------------------------------
// Scaled decode: the picture at 1/2 and 1/4 scale (kernels_dec.hip, launch_scaled).
// ---------------------------------------------------------------------------
extern "C" int himg_hip_scaled_size(int width, int height, int scale_log2, int *ow, int *oh) {
  if (!ow || !oh || width < 1 || height < 1 || (scale_log2 != 1 && scale_log2 != 2)) return HIMG_ERR_ARG;
  const int F = 1 << scale_log2;
  *ow = (int)(((long long)width + F - 1) / F);
  *oh = (int)(((long long)height + F - 1) / F);
  return HIMG_OK;
}

// The device launch behind every scaled entry point.  d_row_index: the host's index (one frame).
static int scaled_launch(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_sizes, int batch,
                         int width, int height, int num_channels, int scale_log2, const uint32_t *d_row_index,
                         void *d_out, int32_t *d_status, void *stream) {
  if (scale_log2 != 1 && scale_log2 != 2) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1 or 2");
  Geom g;
  const uint32_t *d_sizes = nullptr;
  if (int rc = decode_args(ctx, width, height, num_channels, batch, kWsRegion, d_packed, d_out, &in_stride, nullptr, &g))
    return rc;
  // (the region decode's workspace: no FRES plane)
  if (int rc = decode_begin(ctx, g, batch, kWsRegion, h_sizes, stream, &d_sizes)) return rc;
  launch_scaled(g, ctx->dec_ws, batch, (const uint8_t *)d_packed, in_stride, d_sizes, d_row_index, scale_log2,
                (uint8_t *)d_out, d_status, (hipStream_t)stream, &ctx->prof, ctx->opts.use_side ? &ctx->dstr : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_decode_scaled_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                             const uint32_t *h_sizes, int batch, int width, int height,
                                             int num_channels, int scale_log2, void *d_out, int32_t *d_status,
                                             void *stream) {
  if (!ctx || !d_packed || !h_sizes || !d_out || !d_status || batch < 1 || batch > 65535) return HIMG_ERR_ARG;
  if (int rc = stride_covers(ctx, h_sizes, batch, in_stride)) return rc;
  return scaled_launch(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, scale_log2, nullptr, d_out,
                       d_status, stream);
}

// ---------------------------------------------------------------------------
// Picture pyramid: the full, 1/2-, 1/4- and 1/8-scale pictures from one pass (include/himg_hip.h).
// The levels' pointers ride in the kernel arguments of the pyramid forms of the store kernels
// (kernels_dec.hip, launch_decode); level 0 alone is the full decode itself.
// ---------------------------------------------------------------------------
extern "C" int himg_hip_pyramid_size(int width, int height, int level, int *ow, int *oh) {
  if (!ow || !oh || width < 1 || height < 1 || level < 0 || level > 3) return HIMG_ERR_ARG;
  const int F = 1 << level;
  *ow = (int)(((long long)width + F - 1) / F);
  *oh = (int)(((long long)height + F - 1) / F);
  return HIMG_OK;
}

extern "C" int himg_hip_decode_pyramid_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                              const uint32_t *h_sizes, int batch, int width, int height,
                                              int num_channels, const himg_hip_pyramid *out, int32_t *d_status,
                                              void *stream) {
  if (!ctx || !d_packed || !h_sizes || !out || !d_status || batch < 1 || batch > 65535) return HIMG_ERR_ARG;
  himg_dev::PyrDesc pm;
  int wanted = 0;
  const char *bad = nullptr;
  for (int k = 0; k < 4; ++k) {
    pm.level[k] = (uint8_t *)out->level[k];
    if (out->level[k]) ++wanted;
    if ((uintptr_t)out->level[k] & 15) bad = "buffers must be 16-byte aligned";
  }
  if (!wanted) return fail(ctx, HIMG_ERR_ARG, "no pyramid level wanted");
  // (level 0 alone: the full decode, in its own kernels)
  const bool only0 = wanted == 1 && pm.level[0];
  return decode_full(ctx, d_packed, in_stride, h_sizes, batch, width, height, num_channels, pm.level[0], d_status, stream,
                     bad, only0 ? himg_dev::StoreForm() : himg_dev::StoreForm(&pm));
}

// One host stream: stage_whole (the device walks the row headers), one launch, stage_verdict, then a
// piece per wanted level.  The levels lie one behind the other in the output staging, each at a
// multiple of 256 bytes.
extern "C" int himg_hip_decode_pyramid_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                                          uint8_t *const dst[4], const size_t dst_cap[4], int *width, int *height,
                                          int *channels) {
  if (!ctx || !packed || !dst || !dst_cap || !width || !height || !channels) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, &W, &H, &C, &g)) return rc;
  Piece pc[4];
  int wanted = 0, level[4];
  size_t total = 0;
  for (int k = 0; k < 4; ++k) {
    if (!dst[k] && !dst_cap[k]) continue;
    int ow = 0, oh = 0;
    (void)himg_hip_pyramid_size(W, H, k, &ow, &oh);
    pc[wanted] = {total, (size_t)ow * oh * C, dst[k], dst_cap[k]};
    total += round_up(pc[wanted].bytes, 256);
    level[wanted++] = k;
  }
  // (the dimensions and the capacity rule in front of the launch; no level wanted: the dimensions alone)
  if (int rc = out_check(ctx, W, H, C, width, height, channels, pc, wanted)) return rc;
  if (!wanted) return fail(ctx, HIMG_ERR_ARG, "no pyramid level wanted");
  // (nothing stays resident: no fetch_last behind this call)
  if (int rc = stage_whole(ctx, packed, packed_size, total, 4)) return rc;
  himg_hip_pyramid py = himg_hip_pyramid();
  for (int i = 0; i < wanted; ++i) py.level[level[i]] = (uint8_t *)ctx->h_out.p + pc[i].at;
  const uint32_t sz32 = (uint32_t)packed_size;
  int rc = himg_hip_decode_pyramid_device(ctx, ctx->h_in.p, stage_slot(packed_size), &sz32, 1, W, H, C, &py,
                                          (int32_t *)ctx->h_status.p, nullptr);
  int32_t st = 0;
  if ((rc = stage_verdict(ctx, rc, &st, 1))) return rc;
  return pieces_copy(ctx, pc, wanted);
}

// The planes of one host stream: stage_whole (the device walks the row headers), one launch,
// stage_verdict, then deliver's capacity rule and one copy.
extern "C" int himg_hip_decode_planes_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                                         uint32_t plane_mask, uint8_t *dst, size_t dst_cap, int *width, int *height,
                                         int *num_channels) {
  if (!ctx || !packed || !width || !height || !num_channels) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, &W, &H, &C, &g)) return rc;
  if (!plane_mask_ok(C, plane_mask)) return fail(ctx, HIMG_ERR_ARG, "bad plane mask");
  const size_t out_bytes = (size_t)himg_dev::plane_count(plane_mask) * (size_t)W * (size_t)H;
  if (int rc = stage_whole(ctx, packed, packed_size, out_bytes, 4)) return rc;
  const uint32_t sz32 = (uint32_t)packed_size;
  int rc = himg_hip_decode_planes_device(ctx, ctx->h_in.p, stage_slot(packed_size), &sz32, 1, W, H, C, plane_mask,
                                         ctx->h_out.p, (int32_t *)ctx->h_status.p, nullptr);
  int32_t st = 0;
  if ((rc = stage_verdict(ctx, rc, &st, 1))) return rc;
  const Piece pc = {0, out_bytes, dst, dst_cap};
  return deliver(ctx, W, H, C, width, height, num_channels, 0, &pc, 1);   // (not resident: no fetch_last)
}

// ---------------------------------------------------------------------------
// Preview, region and scaled decodes of streams in host memory: streams of one geometry go through the
// staging into one of the device launches above.
// ---------------------------------------------------------------------------
// A launch takes at most kStageLaunch frames (the grids take batch x C <= 65535); the region and scaled
// batches keep its staging within kRegionStageBytes (one frame at least).  A stream occupies its whole
// size there, rounded up to the launch's stride (the largest of its streams): of a region's stream only
// the plan is uploaded, but the kernels bound their reads by the stream's size, so the rest of it must
// be addressable.  Windows near the bottom of large frames are what fill it: their plans end near the
// end of the stream.
constexpr int kStageLaunch = 256;
constexpr size_t kRegionStageBytes = (size_t)1 << 30;

// What the staged entry points differ in, and one call's streams by frame.
struct Staged {
  enum Kind { kPreview, kRegion, kScaled } kind;
  int scale_log2;       // kRegion: 0 (full resolution), 1, 2; kScaled: 1, 2
  bool index;           // the host's row index goes up with the streams (kRegion: and of a stream only its plan)
  const uint8_t *const *packed;
  const size_t *packed_sizes;
  const size_t *heads;    // kPreview: the bytes of a stream that go up (else all of it)
  const int32_t *rects;   // kRegion: (x, y, w, h), in the picture at the scale
};

// A frame's output size: of geometry W x H, for kRegion the window of frame i.
static void staged_dims(const Staged &c, int W, int H, int i, int *ow, int *oh) {
  if (c.kind == Staged::kRegion) { *ow = c.rects[4 * (size_t)i + 2]; *oh = c.rects[4 * (size_t)i + 3]; }
  else if (c.kind == Staged::kScaled) (void)himg_hip_scaled_size(W, H, c.scale_log2, ow, oh);
  else { *ow = (W + 7) / 8; *oh = (H + 7) / 8; }
}

static const char *staged_what(const Staged &c) {
  return c.kind == Staged::kPreview ? "device preview reported an error" : kDecodeError;
}

// Frames grp[0 .. m) -- one geometry, for kRegion one window size, every rectangle checked -- into the
// staging at a stride, one device launch, their statuses to st (what: stage_verdict's, the message of a
// call of one stream or nullptr for a batch).  A stream goes up to its head (kPreview)
// or whole, the rest of its slot zeroed; with the host's index a region's stream only as its plan (the
// head and the touched rows, each at its offset).  A stream the host does not index (a call of its own:
// the batches plan their frames first) goes up whole and takes the device walk, which words the verdict.
static int staged_launch(himg_hip_ctx *ctx, const Staged &c, int W, int H, int C, const int *grp, int m, int32_t *st,
                         const char *what) {
  const int rows = (H + 7) / 8;
  int ow = 0, oh = 0;
  staged_dims(c, W, H, grp[0], &ow, &oh);
  size_t stride = 0;
  for (int k = 0; k < m; ++k) {
    const size_t n = c.heads ? c.heads[grp[k]] : c.packed_sizes[grp[k]];
    stride = n > stride ? n : stride;
  }
  stride = stage_slot(stride);
  const size_t n_idx = c.index ? 2 * (size_t)rows * m : 0, out_bytes = (size_t)ow * oh * C;
  if (int rc = stage_reserve(ctx, ctx->h_in, stride * m, out_bytes * m, (size_t)m * 4, n_idx)) return rc;
  uint8_t *in = (uint8_t *)ctx->h_in.p;
  std::vector<uint32_t> sz(m);
  std::vector<int32_t> org(2 * (size_t)m);
  bool indexed = c.index && rows >= 2;
  for (int k = 0; k < m; ++k) {
    const int i = grp[k];
    sz[k] = (uint32_t)c.packed_sizes[i];
    int up[4] = {0, 0, W, H};   // (kScaled: every row, the whole frame as a rectangle)
    if (c.rects) {
      const int32_t *R = c.rects + 4 * (size_t)i;
      (void)rect_up(W, H, c.scale_log2, R[0], R[1], R[2], R[3], up);
      org[2 * k] = R[0];
      org[2 * k + 1] = R[1];
    }
    himg_hip_region_plan plan = himg_hip_region_plan();
    indexed = indexed && region_index(c.packed[i], c.packed_sizes[i], ctx->fix_t2, up[0], up[1], up[2], up[3], &plan,
                                      ctx->hp_index + (size_t)k * 2 * rows) == HIMG_OK;
    const bool planned = indexed && c.kind == Staged::kRegion;
    const size_t ranges[4] = {0, plan.head_bytes, plan.rows_begin, plan.rows_end};
    if (int rc = stage_upload(ctx, in + (size_t)k * stride, stride, c.packed[i], c.heads ? c.heads[i] : c.packed_sizes[i],
                              planned ? ranges : nullptr, planned ? 2 : 0))
      return rc;
  }
  if (indexed)
    if (int rc = stage_index(ctx, n_idx)) return rc;
  const uint32_t *d_index = indexed ? (const uint32_t *)ctx->h_index.p : nullptr;
  int32_t *d_status = (int32_t *)ctx->h_status.p;
  int rc;
  if (c.kind == Staged::kPreview)
    rc = preview_launch(ctx, in, stride, sz.data(), m, W, H, C, ctx->h_out.p, d_status, nullptr);
  else if (c.kind == Staged::kScaled)
    rc = scaled_launch(ctx, in, stride, sz.data(), m, W, H, C, c.scale_log2, d_index, ctx->h_out.p, d_status, nullptr);
  else
    rc = region_launch(ctx, in, stride, sz.data(), m, W, H, C, org.data(), ow, oh, d_index, ctx->h_out.p, d_status, nullptr,
                       c.scale_log2);
  return stage_verdict(ctx, rc, st, (size_t)m, what);
}

// A *_to call is a launch of one stream (the arrays of c hold that one) whose result stays resident for
// himg_hip_fetch_last; the dimensions are reported even where dst is too small.
static int staged_to(himg_hip_ctx *ctx, const Staged &c, int W, int H, int C, uint8_t *dst, size_t dst_cap, int *width,
                     int *height, int *channels) {
  const int frame = 0;
  int32_t st = 0;
  if (int rc = staged_launch(ctx, c, W, H, C, &frame, 1, &st, staged_what(c))) return rc;
  int ow = 0, oh = 0;
  staged_dims(c, W, H, 0, &ow, &oh);
  const Piece pc = {0, (size_t)ow * oh * C, dst, dst_cap};
  return deliver(ctx, ow, oh, C, width, height, channels, pc.bytes, &pc, 1);
}

// The launches of a batch call.  Frames not yet done that share (W, H, C) -- for kRegion the window size
// too -- go through one launch, in the order of their first frame: at most kStageLaunch of them, whose
// streams, each at the launch's largest size, fit byte_cap (0: no limit).  A failing frame fails alone:
// its dimensions stay zero and the call's first error is kept in *first_err.
static int staged_batch(himg_hip_ctx *ctx, const Staged &c, int n, const int *W, const int *H, const int *C,
                        std::vector<int> &done, size_t byte_cap, uint8_t *const *dst, const size_t *dst_cap, int *widths,
                        int *heights, int *channels, int *first_err) {
  for (int i0 = 0; i0 < n; ++i0) {
    if (done[i0]) continue;
    int ow = 0, oh = 0;
    staged_dims(c, W[i0], H[i0], i0, &ow, &oh);
    const int lim = kStageLaunch < 65535 / C[i0] ? kStageLaunch : 65535 / C[i0];
    std::vector<int> grp;
    size_t stride = 0;
    for (int i = i0; i < n && (int)grp.size() < lim; ++i) {
      int wi = ow, hi = oh;
      if (c.rects) staged_dims(c, W[i], H[i], i, &wi, &hi);
      if (done[i] || W[i] != W[i0] || H[i] != H[i0] || C[i] != C[i0] || wi != ow || hi != oh) continue;
      const size_t si = stage_slot(c.packed_sizes[i]), s2 = si > stride ? si : stride;
      if (byte_cap && !grp.empty() && s2 * (grp.size() + 1) > byte_cap) break;
      stride = s2;
      grp.push_back(i);
      done[i] = 1;
    }
    const int m = (int)grp.size();
    const size_t out_bytes = (size_t)ow * oh * C[i0];
    std::vector<int32_t> st(m);
    if (int rc = staged_launch(ctx, c, W[i0], H[i0], C[i0], grp.data(), m, st.data(), nullptr)) return rc;
    for (int k = 0; k < m; ++k) {
      const int i = grp[k];
      const Piece pc = {(size_t)k * out_bytes, out_bytes, dst[i], dst_cap[i]};
      const int err = st[k] ? status_error(ctx, st[k], staged_what(c)) : pieces_fit(ctx, &pc, 1);
      if (err) { if (!*first_err) *first_err = err; continue; }
      HIP_TRY(ctx, hipMemcpyAsync(dst[i], (uint8_t *)ctx->h_out.p + (size_t)k * out_bytes, out_bytes,
                                  hipMemcpyDeviceToHost, nullptr));
      widths[i] = ow; heights[i] = oh; channels[i] = C[i0];
    }
    HIP_TRY(ctx, hipStreamSynchronize(nullptr));
  }
  return HIMG_OK;
}

extern "C" int himg_hip_preview_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, uint8_t *dst,
                                   size_t dst_cap, int *pw, int *ph, int *channels) {
  if (!ctx || !packed || !pw || !ph || !channels) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  size_t head = 0;
  const char *msg = nullptr;
  // (avail = packed_size: the walk stops at the end of LRES, so the caller's bytes behind it are never read)
  const int rc = preview_walk(packed, packed_size, packed_size, &W, &H, &C, &head, &msg);
  if (rc == HIMG_ERR_FORMAT) return fail(ctx, rc, msg ? msg : "Error decoding low-res data.\n");
  if (rc == HIMG_ERR_UNSUPPORTED) return fail(ctx, rc, "unsupported geometry");
  if (rc) return fail(ctx, rc, "bad stream");
  const Staged c = {Staged::kPreview, 0, false, &packed, &packed_size, &head, nullptr};
  return staged_to(ctx, c, W, H, C, dst, dst_cap, pw, ph, channels);
}

extern "C" int himg_hip_preview_batch(himg_hip_ctx *ctx, const uint8_t *const *packed, const size_t *packed_sizes,
                                      int n, uint8_t *const *dst, const size_t *dst_cap, int *pw, int *ph,
                                      int *channels) {
  if (!ctx || !packed || !packed_sizes || !dst || !dst_cap || !pw || !ph || !channels || n < 0) return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->host_bytes = 0;
  int first_err = HIMG_OK;
  std::vector<int> W(n), H(n), Cc(n), done(n, 0);
  std::vector<size_t> head(n);
  for (int i = 0; i < n; ++i) {
    pw[i] = ph[i] = channels[i] = 0;
    const char *msg = nullptr;
    const int rc = packed[i] ? preview_walk(packed[i], packed_sizes[i], packed_sizes[i], &W[i], &H[i], &Cc[i], &head[i], &msg)
                             : (msg = "Not a RIFF HIMG file.\n", HIMG_ERR_FORMAT);
    if (rc) {
      done[i] = 1;
      if (!first_err) first_err = fail(ctx, rc, msg ? msg : rc == HIMG_ERR_UNSUPPORTED ? "unsupported geometry" : "bad stream");
    }
  }
  // (the staging holds one launch's heads and previews: no byte limit)
  const Staged c = {Staged::kPreview, 0, false, packed, packed_sizes, head.data(), nullptr};
  if (int rc = staged_batch(ctx, c, n, W.data(), H.data(), Cc.data(), done, 0, dst, dst_cap, pw, ph, channels, &first_err))
    return rc;
  return first_err;
}

// himg_hip_decode_region_to (scale_log2 = 0) and himg_hip_decode_scaled_region_to (1, 2: the rectangle
// in the scaled picture, planned as the full-resolution rectangle it covers).  The host walks the headers
// up to the rectangle's last row and uploads the head and the touched rows.
static int region_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int scale_log2, int x, int y,
                     int w, int h, uint8_t *dst, size_t dst_cap, int *width, int *height, int *channels) {
  if (!ctx || !packed || !width || !height || !channels) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0, up[4];
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, &W, &H, &C, &g)) return rc;
  if (!rect_up(W, H, scale_log2, x, y, w, h, up)) return fail(ctx, HIMG_ERR_ARG, "bad rectangle");
  const int32_t R[4] = {x, y, w, h};
  const Staged c = {Staged::kRegion, scale_log2, true, &packed, &packed_size, nullptr, R};
  return staged_to(ctx, c, W, H, C, dst, dst_cap, width, height, channels);
}

extern "C" int himg_hip_decode_region_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int x, int y,
                                         int w, int h, uint8_t *dst, size_t dst_cap, int *width, int *height,
                                         int *channels) {
  return region_to(ctx, packed, packed_size, 0, x, y, w, h, dst, dst_cap, width, height, channels);
}

extern "C" int himg_hip_decode_scaled_region_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                                                int scale_log2, int x, int y, int w, int h, uint8_t *dst,
                                                size_t dst_cap, int *width, int *height, int *channels) {
  if (!ctx) return HIMG_ERR_ARG;
  if (scale_log2 != 1 && scale_log2 != 2) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1 or 2");
  return region_to(ctx, packed, packed_size, scale_log2, x, y, w, h, dst, dst_cap, width, height, channels);
}

// himg_hip_decode_regions_batch (scale_log2 = 0) and himg_hip_decode_scaled_regions_batch (1, 2).
static int regions_batch(himg_hip_ctx *ctx, const uint8_t *const *packed, const size_t *packed_sizes, int n,
                         int scale_log2, const int32_t *rects, uint8_t *const *dst, const size_t *dst_cap, int *widths,
                         int *heights, int *channels) {
  if (!ctx || !packed || !packed_sizes || !rects || !dst || !dst_cap || !widths || !heights || !channels || n < 0)
    return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int first_err = HIMG_OK;
  std::vector<int> W(n), H(n), Cc(n), done(n, 1);
  for (int i = 0; i < n; ++i) {
    widths[i] = heights[i] = channels[i] = 0;
    const int32_t *R = rects + 4 * (size_t)i;
    Geom g;
    int up[4];
    int err = stream_geom(ctx, packed[i], packed_sizes[i], &W[i], &H[i], &Cc[i], &g);
    if (!err && !rect_up(W[i], H[i], scale_log2, R[0], R[1], R[2], R[3], up)) err = fail(ctx, HIMG_ERR_ARG, "bad rectangle");
    if (err) {
      if (!first_err) first_err = err;
      continue;
    }
    himg_hip_region_plan plan = himg_hip_region_plan();
    if (g.rows >= 2 && region_index(packed[i], packed_sizes[i], ctx->fix_t2, up[0], up[1], up[2], up[3], &plan, nullptr) == HIMG_OK) {
      done[i] = 0;   // planned: it goes through a shared launch below
      continue;
    }
    // A stream the host does not index goes through decode_region_to's own path (uploaded whole, the
    // device walk words the verdict), so that its status and message are that call's.
    int w = 0, h = 0, c = 0;
    const int rc = region_to(ctx, packed[i], packed_sizes[i], scale_log2, R[0], R[1], R[2], R[3], dst[i], dst_cap[i],
                             &w, &h, &c);
    if (rc == HIMG_ERR_HIP) return rc;
    if (rc) { if (!first_err) first_err = rc; continue; }
    widths[i] = w; heights[i] = h; channels[i] = c;
  }
  ctx->host_bytes = 0;   // (nothing resident for himg_hip_fetch_last, as in himg_hip_decode_batch)
  const Staged c = {Staged::kRegion, scale_log2, true, packed, packed_sizes, nullptr, rects};
  if (int rc = staged_batch(ctx, c, n, W.data(), H.data(), Cc.data(), done, kRegionStageBytes, dst, dst_cap, widths,
                            heights, channels, &first_err))
    return rc;
  return first_err;
}

extern "C" int himg_hip_decode_regions_batch(himg_hip_ctx *ctx, const uint8_t *const *packed,
                                             const size_t *packed_sizes, int n, const int32_t *rects,
                                             uint8_t *const *dst, const size_t *dst_cap, int *widths, int *heights,
                                             int *channels) {
  return regions_batch(ctx, packed, packed_sizes, n, 0, rects, dst, dst_cap, widths, heights, channels);
}

extern "C" int himg_hip_decode_scaled_regions_batch(himg_hip_ctx *ctx, const uint8_t *const *packed,
                                                    const size_t *packed_sizes, int n, int scale_log2,
                                                    const int32_t *rects, uint8_t *const *dst, const size_t *dst_cap,
                                                    int *widths, int *heights, int *channels) {
  if (!ctx) return HIMG_ERR_ARG;
  if (scale_log2 != 1 && scale_log2 != 2) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1 or 2");
  return regions_batch(ctx, packed, packed_sizes, n, scale_log2, rects, dst, dst_cap, widths, heights, channels);
}

// The windows' plans and the merged, sorted byte ranges of those that have one: [0, head_bytes), then the
// union of their [rows_begin, rows_end).  codes[k]: region_index's for window k; returns the first error.
// One walk serves every window of a sound stream: host_walk to the largest r1_k (to the end of the chunk where
// a window reaches the last block row) with its index of rows [0, r1) -- row r's header starts where row r - 1
// ends, row 0's at head_bytes.  row_index (2 x rows words, or nullptr for scratch of its own) keeps that index.
// Only where that walk fails -- a damaged header chain, which leaves the windows above the break their plans --
// each window is walked on its own.
static int stream_regions_plan(const uint8_t *packed, size_t packed_size, int fix_t2, int n, const int32_t *origins,
                               int w, int h, himg_hip_region_plan *plans, int *codes, std::vector<size_t> *ranges,
                               uint32_t *row_index = nullptr) {
  int first = HIMG_OK, W = 0, H = 0, C = 0;
  size_t head = 0;
  std::vector<std::pair<size_t, size_t>> v;
  const int peek = himg_hip_peek(packed, packed_size, &W, &H, &C);
  const int rows = (H + 7) / 8;
  int rmax = 0;
  for (int k = 0; k < n; ++k) {
    plans[k] = himg_hip_region_plan();
    codes[k] = peek;
    if (peek) continue;
    plans[k].width = W; plans[k].height = H; plans[k].num_channels = C;
    if (!region_ok(W, H, origins[2 * k], origins[2 * k + 1], w, h)) { codes[k] = HIMG_ERR_ARG; continue; }
    plans[k].row0 = origins[2 * k + 1] / 8; plans[k].row1 = (origins[2 * k + 1] + h + 7) / 8;
    rmax = plans[k].row1 > rmax ? plans[k].row1 : rmax;
  }
  std::vector<uint32_t> own;
  if (!row_index && rmax) { own.resize(2 * (size_t)rows); row_index = own.data(); }
  himg_hip_region_plan all = himg_hip_region_plan();
  const bool sound = rmax && host_walk(packed, packed_size, fix_t2, rows, 0, rmax, &all, row_index) == HIMG_OK;
  for (int k = 0; k < n; ++k) {
    if (codes[k] == HIMG_OK && sound) {
      const int r0 = plans[k].row0, r1 = plans[k].row1;
      plans[k].head_bytes = all.head_bytes;
      plans[k].rows_begin = r0 ? (size_t)row_index[r0 - 1] + row_index[rows + r0 - 1] : all.head_bytes;
      plans[k].rows_end = (size_t)row_index[r1 - 1] + row_index[rows + r1 - 1];
    } else if (codes[k] == HIMG_OK) {
      codes[k] = host_walk(packed, packed_size, fix_t2, rows, plans[k].row0, plans[k].row1, &plans[k], nullptr);
    }
    if (plans[k].head_bytes) head = plans[k].head_bytes;
    if (codes[k] == HIMG_OK) v.push_back({plans[k].rows_begin, plans[k].rows_end});
    else if (!first) first = codes[k];
  }
  ranges->clear();
  if (head) v.push_back({0, head});
  std::sort(v.begin(), v.end());
  for (const auto &r : v) {
    if (!ranges->empty() && r.first <= ranges->back()) ranges->back() = r.second > ranges->back() ? r.second : ranges->back();
    else { ranges->push_back(r.first); ranges->push_back(r.second); }
  }
  return first;
}

extern "C" int himg_hip_stream_regions_peek(const uint8_t *packed, size_t packed_size, int fix_t2, int n,
                                            const int32_t *origins, int w, int h, himg_hip_region_plan *plans,
                                            size_t *ranges, int *n_ranges) {
  if (!packed || !origins || !plans || !ranges || !n_ranges || n < 1) return HIMG_ERR_ARG;
  std::vector<int> codes(n);
  std::vector<size_t> r;
  const int rc = stream_regions_plan(packed, packed_size, fix_t2, n, origins, w, h, plans, codes.data(), &r);
  for (int k = 0; k < n; ++k)
    if (codes[k]) {   // (no plan: the geometry if the header gave one, and the window's code)
      plans[k].row0 = codes[k]; plans[k].row1 = 0;
      plans[k].head_bytes = plans[k].rows_begin = plans[k].rows_end = 0;
    }
  memcpy(ranges, r.data(), r.size() * sizeof(size_t));
  *n_ranges = (int)(r.size() / 2);
  return rc;
}

// One host stream, n windows: planned on the host like himg_hip_decode_region_to -- the head and the merged
// ranges of the windows' rows go up, each at its offset, with the host's index of rows [min r0_k, max r1_k) --
// then one launch of stream_regions_launch.  A stream the host does not index for every window (damaged
// headers, one block row) goes up whole and takes the device walk, which gives each window its own verdict.
extern "C" int himg_hip_decode_stream_regions_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int n,
                                                 const int32_t *origins, int w, int h, uint8_t *dst, size_t dst_cap,
                                                 int *statuses, int *width, int *height, int *channels) {
  if (!ctx || !packed || !origins || !statuses || !width || !height || !channels || n < 1 || n > 65535)
    return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, &W, &H, &C, &g)) return rc;
  for (int k = 0; k < n; ++k)
    if (!region_ok(W, H, origins[2 * k], origins[2 * k + 1], w, h)) return fail(ctx, HIMG_ERR_ARG, "bad rectangle");
  const size_t stride = stage_slot(packed_size), out_bytes = (size_t)n * h * w * C, n_idx = 2 * (size_t)g.rows;
  if (int rc = stage_reserve(ctx, ctx->h_in, stride, out_bytes, (size_t)n * 4, n_idx)) return rc;
  std::vector<himg_hip_region_plan> plans(n);
  std::vector<int> codes(n);
  std::vector<size_t> ranges;
  std::vector<int32_t> map(n, 0);
  int32_t index_rows[2] = {g.rows, 0};
  for (int k = 0; k < n; ++k) {
    const int r0 = origins[2 * k + 1] / 8, r1 = (origins[2 * k + 1] + h + 7) / 8;
    index_rows[0] = r0 < index_rows[0] ? r0 : index_rows[0];
    index_rows[1] = r1 > index_rows[1] ? r1 : index_rows[1];
  }
  // (every window planned means the one walk passed: hp_index holds rows [0, max r1_k))
  const bool indexed = g.rows >= 2 && stream_regions_plan(packed, packed_size, ctx->fix_t2, n, origins, w, h, plans.data(),
                                                          codes.data(), &ranges, ctx->hp_index) == HIMG_OK;
  uint8_t *in = (uint8_t *)ctx->h_in.p;
  if (int rc = stage_upload(ctx, in, stride, packed, packed_size, indexed ? ranges.data() : nullptr,
                            indexed ? ranges.size() / 2 : 0))
    return rc;
  if (indexed)
    if (int rc = stage_index(ctx, n_idx)) return rc;
  const uint32_t sz = (uint32_t)packed_size;
  int rc = stream_regions_launch(ctx, in, stride, &sz, 1, W, H, C, map.data(), origins, n, w, h,
                                 indexed ? (const uint32_t *)ctx->h_index.p : nullptr, indexed ? index_rows : nullptr,
                                 ctx->h_out.p, (int32_t *)ctx->h_status.p, nullptr);
  std::vector<int32_t> st(n);
  if ((rc = stage_verdict(ctx, rc, st.data(), (size_t)n, kDecodeError, statuses))) return rc;
  const Piece pc = {0, out_bytes, dst, dst_cap};
  rc = deliver(ctx, w, h, C, width, height, channels, out_bytes, &pc, 1);
  return rc ? rc : first_code(statuses, n);
}

// ---------------------------------------------------------------------------
// Opened streams: the head's products and the rows' records of n streams in memory of their own, and the
// window part of stream_regions_launch alone against them (kernels_dec.hip, launch_open_streams /
// launch_opened_regions; the planning of a call: opened_plan.h).
// ---------------------------------------------------------------------------
struct himg_hip_opened {
  himg_hip_ctx *ctx = nullptr;
  int n_streams = 0, W = 0, H = 0, C = 0, fix_t2 = 0;
  const uint8_t *d_packed = nullptr;   // the caller's (device form) or own_in's (host form)
  size_t in_stride = 0;
  DevBuf mem, own_in;
  DecWs ws{};                          // the handle's buffers; the LRES scratch fields are filled per open
  uint32_t *d_sizes = nullptr;
  himg_dev::OpenedWalk walk{};
  himg_dev::OpenedRows rows;
  hipEvent_t ev = nullptr;             // behind the handle's last call
};
static_assert(sizeof(DecFrame) == 1616, "include/himg_hip.h states a handle's bytes");

// The handle's memory: every array of its own at a 256-byte boundary.  base == nullptr: the size alone.
static size_t opened_carve(const Geom &g, int n_streams, uint8_t *base, himg_hip_opened *o) {
  const size_t n = (size_t)n_streams, rows = (size_t)g.rows;
  const size_t plane = round_up((size_t)g.C * g.rows * g.cols, 256);
  size_t off = 0;
  auto carve = [&](size_t bytes) { size_t at = off; off += round_up(bytes, 256); return base ? base + at : nullptr; };
  uint8_t *frames = carve(n * sizeof(DecFrame)), *nodes = carve(n * 2 * (2 * kNumSym) * 4);
  uint8_t *grp = carve(n * 2 * (1u << kLutBits) * 8), *gyc = carve(n * 2 * (1u << kLutBits) * 4);
  uint8_t *sub = carve(n * 2 * kSubEntries * 8), *index = carve(n * rows * 8), *low = carve(n * plane);
  uint8_t *rec = carve(n * rows * (2 * kDecThreads + himg_dev::kRecHdr) * 4);
  uint8_t *stats = carve((n * (rows + 1) * 8 + n * 4 + n * rows * 8) * 4), *words = carve(n * 12);
  if (o) {
    DecWs &w = o->ws;
    w = DecWs{};
    w.frames = (DecFrame *)frames; w.nodes = (uint32_t *)nodes; w.grp = (uint2 *)grp; w.gyc = (uint32_t *)gyc;
    w.sub = (uint2 *)sub;
    w.row_off = (uint32_t *)index; w.row_len = w.row_off + n * rows;
    w.low = low; w.plane_stride = plane;
    w.lane_start = (uint32_t *)rec; w.lane_off = w.lane_start + n * rows * kDecThreads;
    w.stats = (uint32_t *)stats; w.parse_stats = w.stats + n * (rows + 1) * 8; w.rc_stats = w.parse_stats + n * 4;
    o->d_sizes = (uint32_t *)words;
    o->walk.rows = (int32_t *)words + n; o->walk.st = (int32_t *)words + 2 * n;
  }
  return off;
}

extern "C" int himg_hip_opened_bytes(int width, int height, int num_channels, int n_streams, size_t *bytes) {
  Geom g;
  if (!bytes || n_streams < 1 || n_streams > 65535 || !make_geom(width, height, num_channels, num_channels, 1, &g))
    return HIMG_ERR_ARG;
  *bytes = opened_carve(g, n_streams, nullptr, nullptr);
  return HIMG_OK;
}

static void opened_free(himg_hip_opened *o) {
  if (o->ev) { (void)hipEventSynchronize(o->ev); (void)hipEventDestroy(o->ev); }
  o->mem.release();
  o->own_in.release();
  delete o;
}

static bool opened_owned(const himg_hip_ctx *ctx, const himg_hip_opened *o) {
  if (!ctx || !o) return false;
  for (const himg_hip_opened *p : ctx->opened)   // (no look into o: a closed handle's memory is gone)
    if (p == o) return true;
  return false;
}

// d_row_index: the host's index of all rows (one stream), or nullptr for the device walk.
static int open_streams(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_sizes, int n_streams,
                        int width, int height, int num_channels, const uint32_t *d_row_index, int32_t *d_head_status,
                        DevBuf *own_in, himg_hip_opened **out, void *stream) {
  Geom g;
  const char *bad = nullptr;
  if (height > 0 && num_channels > 0 && ((height + 7) / 8 + 1 > 65535 || (long long)n_streams * num_channels > 65535))
    bad = "grid too large";   // (HIMG_ERR_ARG, as in himg_hip_decode_stream_regions_device)
  if (int rc = decode_args(ctx, width, height, num_channels, n_streams, kWsRegion, d_packed, nullptr, &in_stride, bad, &g))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  himg_hip_opened *o = new himg_hip_opened();
  if (own_in) { o->own_in = *own_in; *own_in = DevBuf(); }
  o->ctx = ctx; o->n_streams = n_streams; o->W = width; o->H = height; o->C = num_channels; o->fix_t2 = g.fix_t2;
  o->d_packed = (const uint8_t *)d_packed; o->in_stride = in_stride;
  o->rows.reset(n_streams, g.rows);
  int rc = HIMG_OK;
  if (!o->mem.reserve(opened_carve(g, n_streams, nullptr, nullptr)) ||
      hipEventCreateWithFlags(&o->ev, hipEventDisableTiming) != hipSuccess)
    rc = fail(ctx, HIMG_ERR_HIP, "opened-streams allocation failed");
  // (the context's workspace in its head-only form: the LRES scratch; everything else is the handle's)
  if (!rc) rc = ensure_dec_ws(ctx, g, n_streams, kWsHead);
  if (!rc) {
    opened_carve(g, n_streams, (uint8_t *)o->mem.p, o);
    ctx->last_stream = (hipStream_t)stream;
    rc = stage_words(ctx, o->d_sizes, h_sizes, (size_t)n_streams, nullptr, 0, ctx->last_stream);
  }
  if (rc) { opened_free(o); return rc; }
  DecWs ws = ctx->dec_ws;
  const DecWs &h = o->ws;
  ws.frames = h.frames; ws.nodes = h.nodes; ws.grp = h.grp; ws.gyc = h.gyc; ws.sub = h.sub;
  ws.row_off = h.row_off; ws.row_len = h.row_len; ws.low = h.low; ws.plane_stride = h.plane_stride;
  ws.lane_start = h.lane_start; ws.lane_off = h.lane_off; ws.lane_q = nullptr;
  ws.stats = h.stats; ws.parse_stats = h.parse_stats; ws.rc_stats = h.rc_stats;
  himg_dev::launch_open_streams(g, ws, n_streams, o->d_packed, in_stride, o->d_sizes, d_row_index, o->walk, d_head_status,
                                (hipStream_t)stream, &ctx->prof, ctx->opts.use_side ? &ctx->dstr : nullptr);
  (void)hipEventRecord(o->ev, (hipStream_t)stream);
  ctx->opened.push_back(o);
  *out = o;
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_open_streams_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                            const uint32_t *h_sizes, int n_streams, int width, int height,
                                            int num_channels, int32_t *d_head_status, himg_hip_opened **out,
                                            void *stream) {
  if (out) *out = nullptr;
  if (!ctx || !d_packed || !h_sizes || !out || n_streams < 1 || n_streams > 65535) return HIMG_ERR_ARG;
  if (int rc = stride_covers(ctx, h_sizes, n_streams, in_stride)) return rc;
  return open_streams(ctx, d_packed, in_stride, h_sizes, n_streams, width, height, num_channels, nullptr, d_head_status,
                      nullptr, out, stream);
}

extern "C" int himg_hip_open_stream_host(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                                         himg_hip_opened **out) {
  if (out) *out = nullptr;
  if (!ctx || !packed || !out) return HIMG_ERR_ARG;
  int W = 0, H = 0, C = 0;
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, &W, &H, &C, &g)) return rc;
  // (the stream's buffer becomes the handle's; the context's h_out and what himg_hip_fetch_last serves stay)
  const size_t stride = stage_slot(packed_size), n_idx = 2 * (size_t)g.rows;
  DevBuf in;
  int rc = stage_reserve(ctx, in, stride, 0, 0, n_idx);
  if (!rc) rc = stage_upload(ctx, (uint8_t *)in.p, stride, packed, packed_size);
  uint32_t first = 0;
  int w2 = 0, h2 = 0, c2 = 0;
  const bool indexed = !rc && g.rows >= 2 &&
                       himg_hip_index_host(packed, packed_size, ctx->fix_t2, &w2, &h2, &c2, ctx->hp_index, (size_t)g.rows,
                                           &first) == HIMG_OK;
  if (indexed) rc = stage_index(ctx, n_idx);
  const uint32_t sz = (uint32_t)packed_size;
  if (!rc)
    rc = open_streams(ctx, in.p, stride, &sz, 1, W, H, C, indexed ? (const uint32_t *)ctx->h_index.p : nullptr, nullptr, &in,
                      out, nullptr);
  (void)hipStreamSynchronize(nullptr);   // the uploads read the caller's and the pinned buffers
  in.release();                          // (open_streams took it over unless it refused)
  return rc;
}

// A call on a handle, every argument checked before anything is launched.  scale_log2 = 0: the windows of the
// full-resolution picture.  1, 2, 3: of the picture at that scale -- ow x oh by himg_hip_scaled_size, and
// ceil(W / 8) x ceil(H / 8) at 3 --, the origins in its coordinates.  At 1 and 2 the planner and the device get the
// origins of the full-resolution rectangles the windows cover, (F x, F y), and the height F h (region_launch's
// rule); at 3 no row is touched, so nothing is planned and the origins go up as they are.
static int opened_launch(himg_hip_ctx *ctx, himg_hip_opened *o, int scale_log2, const int32_t *h_stream_of,
                         const int32_t *h_org, int n_windows, int w, int h, void *d_out, int32_t *d_status, void *stream) {
  if (!opened_owned(ctx, o) || !h_stream_of || !h_org || !d_out || !d_status || n_windows < 1 || n_windows > 65535)
    return HIMG_ERR_ARG;
  if (scale_log2 < 0 || scale_log2 > 3) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1, 2 or 3");
  const int F = 1 << scale_log2;
  const int ow = (int)(((long long)o->W + F - 1) / F), oh = (int)(((long long)o->H + F - 1) / F);
  for (int k = 0; k < n_windows; ++k) {
    if (h_stream_of[k] < 0 || h_stream_of[k] >= o->n_streams) return fail(ctx, HIMG_ERR_ARG, "stream_of outside the streams");
    if (!region_ok(ow, oh, h_org[2 * k], h_org[2 * k + 1], w, h)) return fail(ctx, HIMG_ERR_ARG, "bad rectangle");
  }
  Geom g;
  if (int rc = decode_args(ctx, o->W, o->H, o->C, o->n_streams, kWsRegion, o->d_packed, d_out, nullptr, nullptr, &g)) return rc;
  g.fix_t2 = o->fix_t2;
  ctx->head.valid = false;   // (the words below overwrite the sizes a head phase staged)
  const bool rows_touched = scale_log2 != 3;
  std::vector<int32_t> up_org;
  if (scale_log2 == 1 || scale_log2 == 2) {
    up_org.resize(2 * (size_t)n_windows);
    for (size_t i = 0; i < up_org.size(); ++i) up_org[i] = F * h_org[i];
    h_org = up_org.data();
  }
  // The rows of these windows that no call has counted yet, cut into the count kernels' entries.
  std::vector<himg_dev::OpenedRun> runs;
  const long long list_rows = rows_touched ? o->rows.pending(h_stream_of, h_org, n_windows, F * h, &runs) : 0;
  const size_t o_org = (size_t)n_windows, o_list = o_org + 2 * (size_t)n_windows;
  std::vector<uint32_t> words(o_list);
  memcpy(words.data(), h_stream_of, (size_t)n_windows * 4);
  memcpy(words.data() + o_org, h_org, (size_t)n_windows * 8);
  if (list_rows) himg_dev::opened_cut(runs, himg_dev::stream_count_chunk(g, list_rows), &words);
  const size_t n_list = (words.size() - o_list) / 3;
  if (n_list > 0x7fffffffu) return fail(ctx, HIMG_ERR_UNSUPPORTED, "grid too large");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->d_sizes.reserve(words.size() * 4)) return fail(ctx, HIMG_ERR_HIP, "decoder workspace allocation failed");
  ctx->last_stream = (hipStream_t)stream;
  if (int rc = stage_words(ctx, ctx->d_sizes.p, words.data(), words.size(), nullptr, 0, ctx->last_stream)) return rc;
  o->rows.mark(runs);   // (queued: the stream orders the counts in front of whatever call reads them)
  const int32_t *dw = (const int32_t *)ctx->d_sizes.p;
  if (scale_log2)
    himg_dev::launch_opened_scaled_regions(g, o->ws, o->d_packed, o->in_stride, o->d_sizes, o->walk, scale_log2, dw,
                                           dw + o_org, dw + o_list, n_windows, h_org, (int)n_list, list_rows, w, h,
                                           (uint8_t *)d_out, d_status, (hipStream_t)stream, &ctx->prof);
  else
    himg_dev::launch_opened_regions(g, o->ws, o->d_packed, o->in_stride, o->d_sizes, o->walk, dw, dw + o_org, dw + o_list,
                                    n_windows, h_org, (int)n_list, list_rows, w, h, (uint8_t *)d_out, d_status,
                                    (hipStream_t)stream, &ctx->prof);
  (void)hipEventRecord(o->ev, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_opened_regions_device(himg_hip_ctx *ctx, himg_hip_opened *o, const int32_t *h_stream_of,
                                              const int32_t *h_org, int n_windows, int w, int h, void *d_out,
                                              int32_t *d_status, void *stream) {
  return opened_launch(ctx, o, 0, h_stream_of, h_org, n_windows, w, h, d_out, d_status, stream);
}

extern "C" int himg_hip_opened_scaled_regions_device(himg_hip_ctx *ctx, himg_hip_opened *o, int scale_log2,
                                                     const int32_t *h_stream_of, const int32_t *h_origins, int n_windows,
                                                     int w, int h, void *d_out, int32_t *d_status, void *stream) {
  if (scale_log2 < 1) return opened_owned(ctx, o) ? fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1, 2 or 3") : HIMG_ERR_ARG;
  return opened_launch(ctx, o, scale_log2, h_stream_of, h_origins, n_windows, w, h, d_out, d_status, stream);
}

// The host form of opened_launch (scale_log2 as there).
static int opened_to(himg_hip_ctx *ctx, himg_hip_opened *o, int scale_log2, int n, const int32_t *h_stream_of,
                     const int32_t *origins, int w, int h, uint8_t *dst, size_t dst_cap, int *statuses, int *width,
                     int *height, int *channels) {
  if (!opened_owned(ctx, o) || !origins || !statuses || !width || !height || !channels || n < 1 || n > 65535)
    return HIMG_ERR_ARG;
  if (scale_log2 < 0 || scale_log2 > 3) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1, 2 or 3");
  const int F = 1 << scale_log2;
  const int ow = (int)(((long long)o->W + F - 1) / F), oh = (int)(((long long)o->H + F - 1) / F);
  std::vector<int32_t> map;
  if (!h_stream_of) { map.assign((size_t)n, 0); h_stream_of = map.data(); }
  for (int k = 0; k < n; ++k)
    if (h_stream_of[k] < 0 || h_stream_of[k] >= o->n_streams || !region_ok(ow, oh, origins[2 * k], origins[2 * k + 1], w, h))
      return fail(ctx, HIMG_ERR_ARG, "bad window");
  const size_t out_bytes = (size_t)n * h * w * o->C;
  const Piece pc = {0, out_bytes, dst, dst_cap};
  if (int rc = out_check(ctx, w, h, o->C, width, height, channels, &pc, 1)) return rc;
  // (no stream goes up: the handle holds it.  Nothing stays resident: no fetch_last behind this call.)
  if (int rc = stage_reserve(ctx, ctx->h_in, 0, out_bytes, (size_t)n * 4, 0)) return rc;
  int rc = opened_launch(ctx, o, scale_log2, h_stream_of, origins, n, w, h, ctx->h_out.p, (int32_t *)ctx->h_status.p,
                         nullptr);
  std::vector<int32_t> st(n);
  if ((rc = stage_verdict(ctx, rc, st.data(), (size_t)n, kDecodeError, statuses))) return rc;
  rc = pieces_copy(ctx, &pc, 1);
  return rc ? rc : first_code(statuses, n);
}

extern "C" int himg_hip_opened_regions_to(himg_hip_ctx *ctx, himg_hip_opened *o, int n, const int32_t *h_stream_of,
                                          const int32_t *origins, int w, int h, uint8_t *dst, size_t dst_cap,
                                          int *statuses, int *width, int *height, int *channels) {
  return opened_to(ctx, o, 0, n, h_stream_of, origins, w, h, dst, dst_cap, statuses, width, height, channels);
}

extern "C" int himg_hip_opened_scaled_regions_to(himg_hip_ctx *ctx, himg_hip_opened *o, int scale_log2, int n,
                                                 const int32_t *h_stream_of, const int32_t *origins, int w, int h,
                                                 uint8_t *dst, size_t dst_cap, int *statuses, int *width, int *height,
                                                 int *channels) {
  if (scale_log2 < 1) return opened_owned(ctx, o) ? fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1, 2 or 3") : HIMG_ERR_ARG;
  return opened_to(ctx, o, scale_log2, n, h_stream_of, origins, w, h, dst, dst_cap, statuses, width, height, channels);
}

extern "C" int himg_hip_opened_info(const himg_hip_opened *o, int *n_streams, int *width, int *height, int *channels,
                                    size_t *device_bytes, long long *rows_counted) {
  if (!o) return HIMG_ERR_ARG;
  if (n_streams) *n_streams = o->n_streams;
  if (width) *width = o->W;
  if (height) *height = o->H;
  if (channels) *channels = o->C;
  if (device_bytes) *device_bytes = o->mem.cap + o->own_in.cap;
  if (rows_counted) *rows_counted = o->rows.counted();
  return HIMG_OK;
}

extern "C" void himg_hip_close_streams(himg_hip_ctx *ctx, himg_hip_opened *o) {
  if (!opened_owned(ctx, o)) return;
  for (size_t i = 0; i < ctx->opened.size(); ++i)
    if (ctx->opened[i] == o) { ctx->opened.erase(ctx->opened.begin() + i); break; }
  (void)hipSetDevice(ctx->device);
  opened_free(o);
}

// The host walks every row header (the whole frame as a rectangle) and the index goes up with the
// stream; a stream it does not index takes the device walk, which words the verdict.
extern "C" int himg_hip_decode_scaled_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int scale_log2,
                                         uint8_t *dst, size_t dst_cap, int *width, int *height, int *channels) {
  if (!ctx || !packed || !width || !height || !channels) return HIMG_ERR_ARG;
  if (scale_log2 != 1 && scale_log2 != 2) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1 or 2");
  int W = 0, H = 0, C = 0;
  Geom g;
  if (int rc = stream_geom(ctx, packed, packed_size, &W, &H, &C, &g)) return rc;
  const Staged c = {Staged::kScaled, scale_log2, true, &packed, &packed_size, nullptr, nullptr};
  return staged_to(ctx, c, W, H, C, dst, dst_cap, width, height, channels);
}

// (Every frame's rows are walked on the device: launch_scaled takes the host's index of one frame only.)
extern "C" int himg_hip_decode_scaled_batch(himg_hip_ctx *ctx, const uint8_t *const *packed, const size_t *packed_sizes,
                                            int n, int scale_log2, uint8_t *const *dst, const size_t *dst_cap,
                                            int *widths, int *heights, int *channels) {
  if (!ctx || !packed || !packed_sizes || !dst || !dst_cap || !widths || !heights || !channels || n < 0)
    return HIMG_ERR_ARG;
  if (scale_log2 != 1 && scale_log2 != 2) return fail(ctx, HIMG_ERR_ARG, "scale_log2 must be 1 or 2");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->host_bytes = 0;   // (nothing resident for himg_hip_fetch_last, as in himg_hip_decode_batch)
  int first_err = HIMG_OK;
  std::vector<int> W(n), H(n), Cc(n), done(n, 0);
  for (int i = 0; i < n; ++i) {
    widths[i] = heights[i] = channels[i] = 0;
    Geom g;
    if (const int err = stream_geom(ctx, packed[i], packed_sizes[i], &W[i], &H[i], &Cc[i], &g)) {
      done[i] = 1;
      if (!first_err) first_err = err;
    }
  }
  const Staged c = {Staged::kScaled, scale_log2, false, packed, packed_sizes, nullptr, nullptr};
  if (int rc = staged_batch(ctx, c, n, W.data(), H.data(), Cc.data(), done, kRegionStageBytes, dst, dst_cap, widths,
                            heights, channels, &first_err))
    return rc;
  return first_err;
}

// ---------------------------------------------------------------------------
// Row-sharded encode of one frame over several GPUs (one context per rank).
// ---------------------------------------------------------------------------
extern "C" int himg_hip_shard_stats(himg_hip_ctx *ctx, const void *d_frame_base, int width,
                                    int height, int pixel_stride, int num_channels, int quality,
                                    int use_ycbcr, int row0, int row1, uint32_t *d_fres_hist,
                                    uint8_t *d_low_rows, void *stream) {
  if (!ctx || !d_frame_base || !d_fres_hist || !d_low_rows) return HIMG_ERR_ARG;
  Geom g;
  if (!make_geom(width, height, pixel_stride, num_channels, use_ycbcr, &g))
    return fail(ctx, HIMG_ERR_ARG, "bad geometry");
  // row0 == row1: a rank without rows (more ranks than low-res macro rows) still
  // takes part in every phase; it contributes an all-zero histogram.
  if (row0 < 0 || row1 > g.rows || row0 > row1 || g.rows > 65535)
    return fail(ctx, HIMG_ERR_ARG, "bad block-row range");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // A range of a thousand block rows and more goes through the token stream (k_tok / k_emit_tok: a
  // wavefront per row packs it in ~0.3 ms whatever the number of rows; below, the 1024-lane kernels
  // over the dense plane are faster); HIMG_OPT_ROW_TOKENS forces either.
  const bool shard_tok = ctx->row_tokens != 0 && (ctx->row_tokens > 0 || row1 - row0 >= 1024);
  int rc = ensure_enc_ws(ctx, g, 1, shard_tok, shard_tok);
  if (rc) return rc;
  auto &sh = ctx->shard;
  rc = build_static(g, quality, &sh.sc, &sh.st, &sh.lt);
  if (rc) return fail(ctx, rc, "unsupported table configuration");
  sh.g = g; sh.r0 = row0; sh.r1 = row1; sh.valid = true;
  hipStream_t s = (hipStream_t)stream;
  if (row1 > row0) {
    launch_shard_stats(g, ctx->enc_ws, (const uint8_t *)d_frame_base, sh.st,
                       (const uint8_t *)ctx->fmap_lut.p, row0, row1, s, &ctx->prof);
  } else {
    HIP_TRY(ctx, hipMemsetAsync(ctx->enc_ws.hist, 0, 2 * kHistStride * sizeof(uint32_t), s));
    HIP_TRY(ctx, hipMemsetAsync(ctx->enc_ws.status, 0, sizeof(int32_t), s));
  }
  HIP_TRY(ctx, hipMemcpyAsync(d_fres_hist, ctx->enc_ws.hist + kHistStride, kNumSym * sizeof(uint32_t),
                              hipMemcpyDeviceToDevice, s));
  const size_t n = (size_t)(row1 - row0) * g.cols;
  for (int c = 0; c < g.C; ++c)
    HIP_TRY(ctx, hipMemcpyAsync(d_low_rows + (size_t)c * n,
                                ctx->enc_ws.low + ((size_t)c * g.rows + row0) * g.cols, n,
                                hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_shard_row_bits(himg_hip_ctx *ctx, const uint32_t *d_fres_hist_global,
                                       uint32_t *d_row_bits, void *stream) {
  if (!ctx || !ctx->shard.valid || !d_fres_hist_global || !d_row_bits) return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  auto &sh = ctx->shard;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->enc_ws.hist + kHistStride, d_fres_hist_global,
                              kNumSym * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  launch_shard_row_bits(sh.g, ctx->enc_ws, sh.r0, sh.r1, d_row_bits, s, &ctx->prof);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_shard_emit(himg_hip_ctx *ctx, const uint32_t *d_all_row_bits, void *d_rel,
                                   size_t rel_cap, uint32_t *d_rel_size, void *stream) {
  if (!ctx || !ctx->shard.valid || !d_all_row_bits || !d_rel || !d_rel_size) return HIMG_ERR_ARG;
  if ((rel_cap & 3) || ((uintptr_t)d_rel & 15)) return fail(ctx, HIMG_ERR_ARG, "bad relative buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto &sh = ctx->shard;
  hipStream_t s = (hipStream_t)stream;
  launch_shard_emit(sh.g, ctx->enc_ws, sh.sc, d_all_row_bits, (uint8_t *)d_rel, rel_cap, d_rel_size,
                    sh.r0, sh.r1, s, &ctx->prof);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_shard_assemble(himg_hip_ctx *ctx, const uint8_t *d_low_full,
                                       const uint32_t *d_all_row_bits, const void *d_rel,
                                       size_t rel_bytes, void *d_out, size_t out_cap,
                                       uint32_t *d_size, int32_t *d_status, void *stream) {
  if (!ctx || !ctx->shard.valid || !d_low_full || !d_all_row_bits || !d_rel || !d_out || !d_size)
    return HIMG_ERR_ARG;
  if ((out_cap & 255) || ((uintptr_t)d_out & 15)) return fail(ctx, HIMG_ERR_ARG, "bad output buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto &sh = ctx->shard;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->enc_ws.low, d_low_full, (size_t)sh.g.C * sh.g.rows * sh.g.cols,
                              hipMemcpyDeviceToDevice, s));
  launch_shard_assemble(sh.g, ctx->enc_ws, sh.sc, sh.lt, d_all_row_bits, (const uint8_t *)d_rel,
                        rel_bytes, (uint8_t *)d_out, out_cap, d_size, s, &ctx->prof);
  if (d_status)
    hipLaunchKernelGGL(k_copy_status, dim3(1), dim3(64), 0, s, ctx->enc_ws.status, d_status, 1);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_shard_head(himg_hip_ctx *ctx, const uint8_t *d_low_full, const uint32_t *d_all_row_bits,
                                   void *d_out, size_t out_cap, uint32_t *d_size, uint32_t *d_head,
                                   int32_t *d_status, void *stream) {
  if (!ctx || !ctx->shard.valid || !d_low_full || !d_all_row_bits || !d_out || !d_size || !d_head)
    return HIMG_ERR_ARG;
  if ((out_cap & 255) || ((uintptr_t)d_out & 15)) return fail(ctx, HIMG_ERR_ARG, "bad output buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto &sh = ctx->shard;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->enc_ws.low, d_low_full, (size_t)sh.g.C * sh.g.rows * sh.g.cols,
                              hipMemcpyDeviceToDevice, s));
  launch_shard_head(sh.g, ctx->enc_ws, sh.sc, sh.lt, d_all_row_bits, (uint8_t *)d_out, out_cap, d_size, d_head,
                    sh.r0, sh.r1, s, &ctx->prof);
  if (d_status)
    hipLaunchKernelGGL(k_copy_status, dim3(1), dim3(64), 0, s, ctx->enc_ws.status, d_status, 1);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

extern "C" int himg_hip_shard_finish(himg_hip_ctx *ctx, void *d_out, size_t out_cap, const uint32_t *d_size,
                                     void *stream) {
  if (!ctx || !ctx->shard.valid || !d_out || !d_size) return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_shard_finish(ctx->shard.g, ctx->enc_ws, (uint8_t *)d_out, out_cap, d_size, (hipStream_t)stream, &ctx->prof);
  HIP_TRY(ctx, hipGetLastError());
  return HIMG_OK;
}

// ---------------------------------------------------------------------------
// Introspection.
// ---------------------------------------------------------------------------
extern "C" int himg_hip_debug_read(himg_hip_ctx *ctx, int what, int frame, void *dst,
                                   size_t dst_bytes, size_t *written) {
  if (!ctx || !dst) return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const void *src = nullptr;
  size_t n = 0;
  const bool dec = (what & 0x100) != 0;  // 0x100 | what: decoder-side buffers
  what &= 0xff;
  if (what == HIMG_DBG_LOOP_COUNTS) {
    unsigned long long c[2 * himg_dev::kLoopCounters];
    if (dst_bytes < sizeof(c)) return HIMG_ERR_CAPACITY;
    if ((dec ? himg_dev::loop_counts_read_dec(c) : himg_dev::loop_counts_read_enc(c)) != 0) return HIMG_ERR_ARG;
    memcpy(dst, c, sizeof(c));
    if (written) *written = sizeof(c);
    return HIMG_OK;
  }
  if (!dec) {
    if (!ctx->enc_valid || frame < 0 || frame >= ctx->enc_batch) return HIMG_ERR_ARG;
    const Geom &g = ctx->enc_geom;
    const EncWs &w = ctx->enc_ws;
    const int nsp = g.lres_spans + g.rows;
    switch (what) {
      case HIMG_DBG_AVG: src = w.avg + frame * w.plane_stride; n = (size_t)g.C * g.rows * g.cols; break;
      case HIMG_DBG_LOWRES: src = w.low + frame * w.plane_stride; n = (size_t)g.C * g.rows * g.cols; break;
      case HIMG_DBG_LRES_SYM: src = w.lres_sym + frame * w.lres_stride; n = (size_t)g.lres_size; break;
      case HIMG_DBG_FRES_SYM: src = w.fres_sym + frame * w.fres_stride; n = (size_t)g.fres_size; break;
      case HIMG_DBG_FRES_TOK_SYM: {
        // The token stream of the last batch encode expanded into symbols again (a scratch plane).
        if (!w.tok) return HIMG_ERR_ARG;
        if (!ctx->e_tokx.reserve(round_up((size_t)g.fres_size + 16, 256))) return fail(ctx, HIMG_ERR_HIP, "scratch plane allocation failed");
        himg_dev::launch_tok_expand(g, w, frame, (uint8_t *)ctx->e_tokx.p, nullptr);
        HIP_TRY(ctx, hipDeviceSynchronize());
        src = ctx->e_tokx.p; n = (size_t)g.fres_size; break;
      }
      case HIMG_DBG_TOK_CNT:
        if (!w.tok) return HIMG_ERR_ARG;
        src = w.tok_cnt + (size_t)frame * g.rows * w.tok_nseg; n = (size_t)g.rows * w.tok_nseg * 4; break;
      case HIMG_DBG_LRES_HIST: src = w.hist + ((size_t)frame * 2 + 0) * kHistStride; n = kNumSym * 4; break;
      case HIMG_DBG_FRES_HIST: src = w.hist + ((size_t)frame * 2 + 1) * kHistStride; n = kNumSym * 4; break;
      case HIMG_DBG_LRES_LEN: src = w.lens + ((size_t)frame * 2 + 0) * kHistStride; n = kNumSym * 4; break;
      case HIMG_DBG_FRES_LEN: src = w.lens + ((size_t)frame * 2 + 1) * kHistStride; n = kNumSym * 4; break;
      case HIMG_DBG_LRES_CODE: src = w.codes + ((size_t)frame * 2 + 0) * kHistStride; n = kNumSym * 8; break;
      case HIMG_DBG_FRES_CODE: src = w.codes + ((size_t)frame * 2 + 1) * kHistStride; n = kNumSym * 8; break;
      case HIMG_DBG_FRES_ROW_BYTES: {
        // Convert payload bits to bytes on the host.
        std::vector<uint32_t> bits(g.rows);
        HIP_TRY(ctx, hipMemcpy(bits.data(), w.span_bits + (size_t)frame * nsp + g.lres_spans,
                               (size_t)g.rows * 4, hipMemcpyDeviceToHost));
        n = (size_t)g.rows * 4;
        if (dst_bytes < n) return HIMG_ERR_CAPACITY;
        for (int r = 0; r < g.rows; ++r) ((uint32_t *)dst)[r] = (bits[r] + 7) >> 3;
        if (written) *written = n;
        return HIMG_OK;
      }
      default: return HIMG_ERR_ARG;
    }
  } else {
    if (!ctx->dec_valid || frame < 0 || frame >= ctx->dec_batch) return HIMG_ERR_ARG;
    const Geom &g = ctx->dec_geom;
    const DecWs &w = ctx->dec_ws;
    switch (what) {
      case HIMG_DBG_LOWRES: src = w.low + frame * w.plane_stride; n = (size_t)g.C * g.rows * g.cols; break;
      case HIMG_DBG_LRES_SYM: src = w.lres_sym + frame * w.lres_stride; n = (size_t)g.lres_size; break;
      case HIMG_DBG_FRES_SYM: src = w.fres_sym ? w.fres_sym + frame * w.fres_stride : nullptr; n = (size_t)g.fres_size; break;
      case HIMG_DBG_DEC_STATS: src = w.stats + (size_t)frame * (g.rows + 1) * 8; n = (size_t)(g.rows + 1) * 32; break;
      case HIMG_DBG_PARSE_STATS: src = w.parse_stats + (size_t)frame * 4; n = 16; break;
      case HIMG_DBG_LANE_START: src = w.lane_start ? w.lane_start + (size_t)frame * g.rows * kDecThreads : nullptr; n = (size_t)g.rows * kDecThreads * 4; break;
      case HIMG_DBG_LANE_OFF:
        src = w.lane_off ? w.lane_off + (size_t)frame * g.rows * (kDecThreads + himg_dev::kRecHdr) : nullptr;
        n = (size_t)g.rows * (kDecThreads + himg_dev::kRecHdr) * 4; break;
      case HIMG_DBG_ROWCOUNT_STATS: src = w.rc_stats ? w.rc_stats + (size_t)frame * g.rows * 8 : nullptr; n = (size_t)g.rows * 32; break;
      default: return HIMG_ERR_ARG;
    }
    if (!src) return HIMG_ERR_ARG;   // (after a preview: the workspace holds no FRES side)
  }
  if (dst_bytes < n) return HIMG_ERR_CAPACITY;
  HIP_TRY(ctx, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
  if (written) *written = n;
  return HIMG_OK;
}

extern "C" int himg_hip_debug_trees(himg_hip_ctx *ctx, const uint32_t *hist, int n, uint64_t *codes,
                                    uint32_t *lens, uint8_t *trees, uint32_t *tree_bytes, int32_t *status) {
  if (!ctx || !hist || !codes || !lens || !trees || !tree_bytes || !status || n < 1 || n > 16384) return HIMG_ERR_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  // The workspace as k_tree expects it: [frame][2 slots][padded row]; nothing else of an EncWs is read.
  const size_t slots = (size_t)n * 2;
  size_t total = 0;
  auto carve = [&](size_t bytes) { const size_t o = total; total += round_up(bytes, 256); return o; };
  const size_t o_hist = carve(slots * kHistStride * 4), o_codes = carve(slots * kHistStride * 8);
  const size_t o_lens = carve(slots * kHistStride * 4), o_tree = carve(slots * kTreeStride);
  const size_t o_nb = carve(slots * 4), o_status = carve((size_t)n * 4);
  if (!ctx->e_dbgtree.reserve(total)) return fail(ctx, HIMG_ERR_HIP, "tree scratch allocation failed");
  uint8_t *base = (uint8_t *)ctx->e_dbgtree.p;
  EncWs w{};
  w.hist = (uint32_t *)(base + o_hist);
  w.codes = (uint64_t *)(base + o_codes);
  w.lens = (uint32_t *)(base + o_lens);
  w.tree = base + o_tree;
  w.tree_nbytes = (uint32_t *)(base + o_nb);
  w.status = (int32_t *)(base + o_status);
  std::vector<uint32_t> h(slots * kHistStride, 0u);
  for (size_t s = 0; s < slots; ++s) memcpy(&h[s * kHistStride], hist + (s / 2) * kNumSym, kNumSym * 4);
  HIP_TRY(ctx, hipMemset(base, 0, total));
  HIP_TRY(ctx, hipMemcpy(w.hist, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  himg_dev::launch_debug_trees(w, n, nullptr);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipDeviceSynchronize());
  std::vector<uint64_t> c(slots * kHistStride);
  std::vector<uint8_t> t(slots * kTreeStride);
  HIP_TRY(ctx, hipMemcpy(c.data(), w.codes, c.size() * 8, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(h.data(), w.lens, h.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(t.data(), w.tree, t.size(), hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(tree_bytes, w.tree_nbytes, slots * 4, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(status, w.status, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (size_t s = 0; s < slots; ++s) {
    memcpy(codes + s * kNumSym, &c[s * kHistStride], kNumSym * 8);
    memcpy(lens + s * kNumSym, &h[s * kHistStride], kNumSym * 4);
    memcpy(trees + s * kTreeStride, &t[s * kTreeStride], kTreeStride);
  }
  return HIMG_OK;
}

extern "C" int himg_hip_profile_enable(himg_hip_ctx *ctx, int enable) {
  if (!ctx) return HIMG_ERR_ARG;
  ctx->prof.enabled = enable != 0;
  return HIMG_OK;
}

extern "C" int himg_hip_profile_reset(himg_hip_ctx *ctx) {
  if (!ctx) return HIMG_ERR_ARG;
  hipSetDevice(ctx->device);
  ctx->prof.collect();
  ctx->prof.acc.clear();
  return HIMG_OK;
}

extern "C" int himg_hip_profile_read(himg_hip_ctx *ctx, int *n_stages,
                                     const char *names[HIMG_MAX_STAGES],
                                     double ms[HIMG_MAX_STAGES], int launches[HIMG_MAX_STAGES]) {
  if (!ctx || !n_stages) return HIMG_ERR_ARG;
  hipSetDevice(ctx->device);
  ctx->prof.collect();
  int n = 0;
  for (auto &a : ctx->prof.acc) {
    if (n >= HIMG_MAX_STAGES) break;
    names[n] = a.name.c_str();
    ms[n] = a.ms;
    launches[n] = a.n;
    ++n;
  }
  *n_stages = n;
  return HIMG_OK;
}
