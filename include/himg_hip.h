/*
 * himg_hip.h -- C ABI of the MI355X-native HIMG encode/decode engine.
 *
 * This is the drop-in boundary: plain C, pointers and sizes
 * only, int status returns, no C++/torch types.  The reference has no FFI of
 * its own; the interface a binding would wrap is the public surface of
 *   himg::Encoder  (reference src/lib/encoder.h:20-64, encoder.cpp:59-109)
 *   himg::Decoder  (reference src/lib/decoder.h:22-67, decoder.cpp:87-138)
 * and every entry point below names the member it replaces.  The C++ classes
 * in include/encoder.h / include/decoder.h are thin wrappers over this ABI, so
 * reference callers (src/chimg.cpp:140-163, src/dhimg.cpp:45-65,
 * src/benchmark.cpp:108-125) compile unchanged.
 *
 * All device work is hand-written HIP for gfx950; there is NO CPU fallback:
 * without a usable GPU every compute entry point returns HIMG_ERR_HIP.
 */
#ifndef HIMG_HIP_H_
#define HIMG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define HIMG_OK 0
#define HIMG_ERR_ARG (-1)         /* bad argument */
#define HIMG_ERR_HIP (-2)         /* HIP runtime failure / no device */
#define HIMG_ERR_UNSUPPORTED (-3) /* geometry or stream outside the built scope */
#define HIMG_ERR_FORMAT (-4)      /* decode: the reference would return false */
#define HIMG_ERR_CAPACITY (-5)    /* output buffer too small */
#define HIMG_ERR_TARGET (-6)      /* encode to a distortion target: not reached at the highest quality */
/* One deviation from the reference decoder: a Huffman tree (LRES or FRES) with a leaf more than 32
 * branches below the root is answered with HIMG_ERR_UNSUPPORTED by every decode entry point.  The
 * reference decodes such a stream; its encoder cannot write one (it keeps codes in 32 bits). */

typedef struct himg_hip_ctx himg_hip_ctx;

/* One context per device per host thread.  It owns the device workspace
 * (intermediate planes, symbol buffers, scan scratch) sized lazily for the
 * largest geometry/batch seen.  Not re-entrant; distinct contexts are
 * independent (mirrors "distinct Decoder objects are independent",
 * decoder.cpp:292-326). */
int himg_hip_create(int device, himg_hip_ctx **ctx);
void himg_hip_destroy(himg_hip_ctx *ctx);
const char *himg_hip_last_error(const himg_hip_ctx *ctx);

/* Options (default 0 = behave exactly like the reference).
 * HIMG_OPT_FIX_T2: the reference DECODER cannot read two kinds of streams its own
 * encoder writes: (i) highly compressible ones -- it derives "the stream is split
 * into blocks" from the COMPRESSED size (huffman_dec.cpp:215-219) while the
 * encoder decides on the uncompressed size (huffman_enc.cpp:256), so flat or
 * smooth frames are rejected (SURVEY.md trap T2), as is every frame of at most 8
 * pixel rows; (ii) streams whose token alphabet is one symbol -- written with
 * 1-bit codes (huffman_enc.cpp:231-237), read with 0 bits.  With the option set the
 * decoder applies the encoder's rules and decodes them; streams the reference
 * accepts decode identically either way.  Also enabled by HIMG_FIX_T2=1 in the
 * environment (for callers that only see the C++ classes). */
#define HIMG_OPT_FIX_T2 1
/* Kernel-variant selectors (tuning / test knobs; results are identical either way).
 * value -1 = by launch size (the default), 0 / 1 = force off / on:
 *   HIMG_OPT_COUNT_WAVE  FRES row index records by a wavefront per row (batches) instead of
 *                        a workgroup per row (single frames)            [env HIMG_COUNT_WAVE]
 *   HIMG_OPT_EMIT_ROWS   bit packing of FRES rows by a wavefront per row (batches) [env HIMG_EMIT_ROWS]
 *   HIMG_OPT_ROW_TOKENS  encoder: FRES rows go from the tokeniser to the bit packer as a stream of 16-bit
 *                        tokens (k_tok / k_emit_tok) instead of both walking the dense symbol plane (batches);
 *                        value 2 = on, and the bit packer takes its spelled-out path on every step (a test knob)
 *                        Rows so wide that k_tok's stage could overflow (himg_hip_tok_layout: above 21 864
 *                        RGBA pixels) keep the dense plane whatever the value.
 *                                                                      [env HIMG_ROW_TOKENS]
 *   HIMG_OPT_FRONT       encoder, full RGBA8 frames with rows of at most 512 tiles: box averages, low-res
 *                        plane and pixel stage in ONE pass over the pixels (k_front) instead of three
 *                        kernels reading them twice (batches)               [env HIMG_FRONT] */
#define HIMG_OPT_COUNT_WAVE 2
#define HIMG_OPT_EMIT_ROWS 3
#define HIMG_OPT_ROW_TOKENS 4
#define HIMG_OPT_FRONT 5
/*   HIMG_OPT_COUNT_STRETCH  the wavefront-per-row form of the FRES row index records: consecutive
 *                        sub-sequences of a row that one lane walks as a single stretch -- 2, 4 or 8;
 *                        1 = one each (the earlier form, kept for A/B runs and the tests);
 *                        -1 = the default.  Other values: HIMG_ERR_ARG.     [env HIMG_COUNT_STRETCH] */
#define HIMG_OPT_COUNT_STRETCH 6
int himg_hip_set_option(himg_hip_ctx *ctx, int option, int value);
/* The option as the context holds it -- including what it took from the environment when it
 * was created (HIMG_FIX_T2=1): a binding that mirrors an option (the row-sharded decoder's host
 * index follows HIMG_OPT_FIX_T2) reads it here instead of tracking set_option calls. */
int himg_hip_get_option(himg_hip_ctx *ctx, int option, int *value);

/* Upper bound of the packed size of one frame (bytes), a multiple of 256.
 * Replaces HuffmanEnc::MaxCompressedSize (huffman_enc.cpp:242-244) plus the
 * container overhead of encoder.cpp:111-256. */
size_t himg_hip_max_packed_size(int width, int height, int num_channels);

/* ---- host-buffer API (what the C++ wrapper classes call) ---------------- */

/* Replaces himg::Encoder::Encode + packed_data()/packed_size()
 * (encoder.h:24-34).  `data`: tightly packed rows of width*pixel_stride
 * bytes, channel c of pixel (x,y) at (y*width+x)*pixel_stride+c
 * (encoder.cpp:297).  *out is malloc'ed; release with himg_hip_free.
 * Every call has fresh-Encoder semantics (SURVEY.md trap T4). */
int himg_hip_encode(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                    int pixel_stride, int num_channels, int quality, int use_ycbcr,
                    uint8_t **out, size_t *out_size);

/* Replaces himg::Decoder::Decode + unpacked_data()/width()/height()/
 * num_channels() (decoder.h:26-33).  Returns HIMG_ERR_FORMAT exactly where
 * the reference returns false (including trap T2 streams). *out is malloc'ed
 * width*height*channels bytes. */
int himg_hip_decode(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                    uint8_t **out, int *width, int *height, int *num_channels);

void himg_hip_free(void *p);

/* The same two operations into caller-owned host memory.  A caller that reuses
 * its buffers (the reference's benchmark decodes 30x with one Decoder,
 * benchmark.cpp:122-125) avoids a fresh 64 MiB allocation per call, whose page
 * faults cost several times the PCIe transfer.  HIMG_ERR_CAPACITY (with the
 * required size in *out_size / the geometry in *width...) when dst is too small
 * or NULL; the result then stays resident and himg_hip_fetch_last copies it
 * without repeating the work.  himg_hip_peek reads only the FRMT chunk (no GPU). */
int himg_hip_encode_to(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                       int pixel_stride, int num_channels, int quality, int use_ycbcr,
                       uint8_t *dst, size_t dst_cap, size_t *out_size);
int himg_hip_decode_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, uint8_t *dst,
                       size_t dst_cap, int *width, int *height, int *num_channels);
int himg_hip_fetch_last(himg_hip_ctx *ctx, uint8_t *dst, size_t dst_cap, size_t *size);
int himg_hip_peek(const uint8_t *packed, size_t packed_size, int *width, int *height,
                  int *num_channels);

/* ---- batched host API: frames in flight -------------------------------------- */
/* n frames from / to host memory with the transfers hidden behind the kernels:
 * H2D of frame i+1, the kernels of frame i and D2H of frame i-1 run on three
 * streams over double-buffered staging (reference protocol to mirror:
 * benchmark.cpp:111-149, one picture after the other).  Same per-frame semantics
 * as himg_hip_encode_to / himg_hip_decode_to.  A frame that fails (or whose dst is
 * too small) gets out_sizes[i] = 0 / widths[i] = 0 and does not stop the others;
 * the return value is the first such error, HIMG_OK if there was none.
 * All frames of one encode call share the geometry; decode takes it per frame
 * from the FRMT chunk. */
int himg_hip_encode_batch(himg_hip_ctx *ctx, const uint8_t *const *frames, int n, int width,
                          int height, int pixel_stride, int num_channels, int quality,
                          int use_ycbcr, uint8_t *const *dst, const size_t *dst_cap,
                          size_t *out_sizes);
int himg_hip_decode_batch(himg_hip_ctx *ctx, const uint8_t *const *packed, const size_t *packed_sizes,
                          int n, uint8_t *const *dst, const size_t *dst_cap, int *widths,
                          int *heights, int *channels);

/* Page-locked host memory for the frames / streams handed to the host API: from
 * pinned buffers the transfers above are true asynchronous DMA at PCIe speed and
 * overlap the kernels; from pageable memory the runtime stages every copy.  (The
 * reference's callers own their buffers too: benchmark.cpp:104-105 loads the file
 * into a std::vector once and decodes it 30 times.)  Returns NULL on failure. */
void *himg_hip_host_alloc(size_t bytes);
void himg_hip_host_free(void *p);

/* ---- device-resident batched API (roofline measurements, pipelines) ----- */

/* Streams.  Every entry point of this section and of the device forms below takes the caller's
 * `stream` and is asynchronous: it queues its work and returns; nothing is synchronised with the host
 * (the exceptions: a context's first call at a larger geometry, which reserves workspace; the first call
 * of the per-quality encode section; and, since eight pinned slots carry the host arrays to the device, a
 * call whose slot is still waiting for its copy eight calls back waits for that copy -- not for the
 * kernels behind it).  All of a call's work is ordered on `stream`: it starts
 * behind what the stream held at the call and is complete for whatever the caller queues on the stream
 * afterwards -- the context's own side streams are forked from `stream` and joined back into it before
 * the call returns.  HOST arrays (h_sizes, h_origins, h_quality, ...) are copied before the call
 * returns; the caller may reuse them at once.
 * A context's calls are ordered by the caller's stream ALONE.  The context keeps one workspace and one
 * set of staging buffers for all its calls, so consecutive calls on one stream need no wait between them,
 * and a caller who moves a context from one stream to another orders the two: the new stream waits
 * (hipStreamWaitEvent) for an event recorded on the old one behind the context's last call there, or the
 * host waits for that call.  Calls of one context on two streams without such an order race on the
 * workspace.  Distinct contexts share nothing and may run on distinct streams at the same time.
 * The legacy null stream (stream = NULL) is a stream like any other here; a non-blocking stream is not
 * synchronised with it, and no call queues anything on it on the caller's behalf. */

/* Encode `batch` frames that already live in HBM.
 *   d_frames : device pointer, batch * height*width*pixel_stride bytes
 *   d_out    : device pointer, batch * out_stride bytes (out_stride a multiple
 *              of 256 and >= himg_hip_max_packed_size).  Stream f is the first
 *              d_sizes[f] bytes of slot f (d_out + f * out_stride); the slot's
 *              other bytes are unspecified up to offset
 *              620 + C * (rows * cols + ceil(rows/16) * ceil(cols/16)), rounded
 *              up to 4, rows = ceil(H/8), cols = ceil(W/8) -- the encoder clears
 *              the worst-case extent of the low-res chunk in every slot before
 *              it packs, so a shorter stream is followed by zeros -- and
 *              are not written from there on when the frame succeeds.  Every
 *              encode entry point with a d_out obeys this.
 *   d_sizes  : device pointer, batch x uint32 packed sizes (0 on failure)
 *   d_status : device pointer, batch x int32 (HIMG_OK or an error code)
 *   stream   : hipStream_t (NULL = default stream).  Asynchronous: nothing is
 *              synchronised with the host.  Same per-frame semantics as
 *              himg_hip_encode. */
int himg_hip_encode_device(himg_hip_ctx *ctx, const void *d_frames, int batch,
                           int width, int height, int pixel_stride,
                           int num_channels, int quality, int use_ycbcr,
                           void *d_out, size_t out_stride, uint32_t *d_sizes,
                           int32_t *d_status, void *stream);

/* Decode `batch` streams that already live in HBM; all must have the stated
 * geometry (it is validated on the device against each stream's FRMT chunk).
 *   d_packed : device pointer, stream f starts at d_packed + f*in_stride; in_stride
 *              is a multiple of 4 and >= every packed size rounded up to 4 (the
 *              decoder reads whole dwords)
 *   h_sizes  : HOST array, batch packed sizes
 *   d_out    : device pointer, batch * width*height*num_channels bytes
 *   d_status : device pointer, batch x int32 */
int himg_hip_decode_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                           const uint32_t *h_sizes, int batch, int width, int height,
                           int num_channels, void *d_out, int32_t *d_status,
                           void *stream);

/* ---- quality per frame, and encode to a byte budget --------------------------- */
/*
 * Quality enters the encoder only as small tables (the quantiser's shifts, the low-res companding
 * table, the LMAP and QCFG chunks).  A context keeps them for all 101 qualities in HBM -- built on
 * its first call of this section, the one place where these calls wait for the device -- and the
 * kernels that read them pick frame f's by a quality index on the device.
 */
/* A quality per frame: h_quality is a HOST array of `batch` values in [0, 100] (any other value:
 * HIMG_ERR_ARG, nothing launched, neither d_out nor d_status written); it reaches the device as
 * h_sizes / h_origins do in the decode (no host synchronisation).  Otherwise the contract of
 * himg_hip_encode_device; frame f's bytes are those of himg_hip_encode at quality h_quality[f]. */
int himg_hip_encode_device_q(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                             int pixel_stride, int num_channels, const int32_t *h_quality, int use_ycbcr,
                             void *d_out, size_t out_stride, uint32_t *d_sizes, int32_t *d_status,
                             void *stream);
/* The exact stream size of every frame at its quality, WITHOUT writing a stream: d_sizes[f] is what
 * himg_hip_encode_device_q would report (for any out_stride that obeys its contract); no output
 * buffer, no out_stride, no bit packing -- the size follows from the token histograms and the code
 * lengths.  d_status[f]: a failure of the stages in front of the bit packer (d_sizes[f] is then 0). */
int himg_hip_encode_sizes_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                 int pixel_stride, int num_channels, const int32_t *h_quality,
                                 int use_ycbcr, uint32_t *d_sizes, int32_t *d_status, void *stream);
/*
 * Encode to a byte budget: "at most B bytes for this picture".  Per frame, frames independent of each
 * other; size(q) is the frame's exact stream size at quality q (himg_hip_encode_sizes_device), B its
 * budget in bytes (h_budgets: a HOST array of `batch` values, staged like h_quality):
 *   1. probe qmin.  size(qmin) > B: the frame fails -- d_quality[f] = -1, d_sizes[f] = 0, d_status[f] =
 *      HIMG_ERR_CAPACITY; its bytes in d_out are unspecified but stay inside its out_stride bytes.
 *      The other frames go on.
 *   2. if qmax > qmin, probe qmax.  It fits: the result is qmax.
 *   3. otherwise lo = qmin, hi = qmax; while hi - lo > 1: mid = (lo + hi) >> 1; size(mid) <= B ?
 *      lo = mid : hi = mid.  The result is lo.
 * Every frame with a result is then encoded at it: d_quality[f] holds the result, d_out / d_sizes[f]
 * exactly the bytes and the size of himg_hip_encode at that quality, d_status[f] that encode's status
 * (d_quality[f] = -1 and d_sizes[f] = 0 as well where a probe or the encode itself failed).  The probe's
 * size is exact, so d_sizes[f] <= B.
 * The size is NOT monotone in the quality -- over q = 0 .. 100 most small test pictures have 2 to 17
 * places where size(q + 1) < size(q): random noise shrinks from q = 95 upwards, gradients wobble below
 * q = 30 (tests/test_budget_host.py holds the oracle to it) -- so this is THE SEARCH'S result, a
 * deterministic quality that is guaranteed to fit, not the largest fitting one, which would take all
 * 101 encodes.
 * Asynchronous on the caller's stream, no host synchronisation: every frame takes the launch's fixed
 * number of probes (himg_hip_budget_probes; a settled frame repeats its last one), lo / hi / the next
 * quality live on the device and a small kernel advances them between two probes.  out_stride obeys
 * the contract of himg_hip_encode_device (>= himg_hip_max_packed_size), so a chosen stream always fits.
 */
/* Host only, no GPU: the number of size probes the search makes for [qmin, qmax]: 1 when qmin == qmax,
 * else 2 + ceil(log2(qmax - qmin)) (9 for 0 .. 100); HIMG_ERR_ARG unless 0 <= qmin <= qmax <= 100. */
int himg_hip_budget_probes(int qmin, int qmax);
int himg_hip_encode_budget_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                  int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                                  const uint32_t *h_budgets, void *d_out, size_t out_stride,
                                  uint32_t *d_sizes, int32_t *d_quality, int32_t *d_status, void *stream);
/* The host forms: himg_hip_encode_to / himg_hip_encode_batch with a budget (in bytes; one above 2^32 - 1
 * counts as that) -- the capacity protocol, himg_hip_fetch_last, a failing frame's out_sizes[i] = 0
 * and the first error as the return value, as there.  *quality / qualities[i]: the chosen quality; -1
 * for a frame whose budget is below size(qmin), for which the call returns HIMG_ERR_CAPACITY (the
 * batch form: as that frame's error). */
int himg_hip_encode_budget_to(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                              int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                              size_t budget, uint8_t *dst, size_t dst_cap, size_t *out_size, int *quality);
int himg_hip_encode_budget_batch(himg_hip_ctx *ctx, const uint8_t *const *frames, int n, int width,
                                 int height, int pixel_stride, int num_channels, int qmin, int qmax,
                                 int use_ycbcr, const size_t *budgets, uint8_t *const *dst,
                                 const size_t *dst_cap, size_t *out_sizes, int *qualities);

/* ---- encode windows of pitched source pictures -------------------------------- */
/*
 * The encode entry points above take whole, tightly packed frames.  This one takes a row pitch and a
 * rectangle per frame, the way the region decodes do on the other side: frames from hipMallocPitch or
 * a surface with padded rows, the tiles of one large picture (frame_pitch = 0), or a region of
 * interest per frame are encoded where they lie, without a copy pass that makes them contiguous.
 */
typedef struct himg_hip_src {
  int width, height;      /* the source pictures in pixels: every window lies inside */
  int pixel_stride;       /* bytes from a pixel to the next, >= num_channels */
  size_t row_pitch;       /* bytes from a row to the next, >= width * pixel_stride */
  size_t frame_pitch;     /* bytes from source picture f to f + 1; 0: all windows read ONE picture */
} himg_hip_src;

/* Window f of the batch is the w x h picture whose pixel (i, j), channel c, is the byte at
 *   d_src + f * frame_pitch + (y_f + i) * row_pitch + (x_f + j) * pixel_stride + c,
 * (x_f, y_f) = h_origins[2 f], h_origins[2 f + 1].  Stream f in d_out + f * out_stride, d_sizes[f] and
 * d_status[f] are byte for byte what himg_hip_encode gives for that picture at quality h_quality[f];
 * the low-res sampling clips at the window's edges, not the source's.  Otherwise the contract of
 * himg_hip_encode_device_q: asynchronous, no host synchronisation, the out_stride rule (for the
 * WINDOW's size), the grid limits.  h_origins is a HOST array of 2 * batch values that rides to the
 * device with h_quality, as the decode's origins do with its sizes.  Windows may overlap; with
 * frame_pitch == 0 they all come from one picture.
 *
 * Checks, all on the host before anything is launched -- a failure returns HIMG_ERR_ARG and none of
 * d_out, d_sizes, d_status is written:
 *   - src NULL, or a source or window size that is not positive;
 *   - pixel_stride < num_channels;
 *   - row_pitch < width * pixel_stride;
 *   - frame_pitch neither 0 nor at least (height - 1) * row_pitch + width * pixel_stride;
 *   - a window not inside width x height (x_f, y_f >= 0, x_f + w <= width, y_f + h <= height);
 *   - a quality outside [0, 100];
 *   - d_src not 16-byte aligned;
 *   - for pixel_stride == 4: row_pitch or frame_pitch not a multiple of 4.
 * The origins themselves are unconstrained: an odd x_f is legal (the kernels load a window's tile rows
 * at pixel alignment).
 *
 * Bytes used: only the windows' own pixels decide the result, and nothing at or beyond *bytes of
 * himg_hip_windows_extent is loaded: the largest
 *   f * frame_pitch + (y_f + h - 1) * row_pitch + (x_f + w) * pixel_stride
 * over the batch -- a buffer may end with its last window's last pixel.
 *
 * Not in this change: windows for the size probe (himg_hip_encode_sizes_device), for the distortion
 * probe (its comparison kernel reads the source too), for the two searches, for the row-sharded and
 * multi-GPU paths; a batch host form; the C++ classes. */
/* Host only, no GPU: the checks above (those of src, the window size and the origins; num_channels in
 * 1 .. 4), the same codes, and *bytes. */
int himg_hip_windows_extent(const himg_hip_src *src, int num_channels, int batch,
                            const int32_t *h_origins, int w, int h, size_t *bytes);
int himg_hip_encode_windows_device(himg_hip_ctx *ctx, const void *d_src, const himg_hip_src *src,
                                   int batch, int num_channels, const int32_t *h_origins, int w, int h,
                                   const int32_t *h_quality, int use_ycbcr, void *d_out, size_t out_stride,
                                   uint32_t *d_sizes, int32_t *d_status, void *stream);
/* One window (x, y, w, h) of a HOST picture described by src (frame_pitch is ignored): only rows
 * [y, y + h) of the source are uploaded, one contiguous range, and encoded by the device form with
 * batch 1 and origin (x, 0).  The capacity protocol and himg_hip_fetch_last as himg_hip_encode_to. */
int himg_hip_encode_window_to(himg_hip_ctx *ctx, const uint8_t *data, const himg_hip_src *src,
                              int num_channels, int x, int y, int w, int h, int quality, int use_ycbcr,
                              uint8_t *dst, size_t dst_cap, size_t *out_size);

/* ---- the distortion of an encode, and encode to a distortion target ----------- */
/*
 * sse(q) of a frame: the sum over all H x W x C samples of (source - decoded)^2, where `decoded` is
 * the decode of himg_hip_encode at quality q with HIMG_OPT_FIX_T2 on.  Only real pixels count (for
 * W % 8 != 0 or H % 8 != 0 the clipped picture, as the decoder defines it), and of every pixel_stride
 * bytes only the first num_channels.  An exact integer in a uint64_t (16384^2 RGBA: at most 7e13).
 * Why the fixed decode: the reference decoder rejects many of its own encoder's streams (trap T2) --
 * 327 of the 808 streams of eight small pictures over q = 0 .. 100 without the fix, none with it -- and
 * wherever it accepts one its pixels equal the fixed decode's, so the fixed decode is the picture the
 * stream defines.  The definition does not depend on the context's own HIMG_OPT_FIX_T2.
 *
 * The probe computes it without an entropy coder in either direction: the encoder's front stages
 * leave every frame's quantised symbols and low-res plane on the device; the low-res chain stores
 * the samples it reconstructs while it codes (what a decoder gets back), and one kernel sends the
 * symbols through the decoder's dequantiser, inverse transform, low-res add, clamp and inverse
 * colour transform and compares the result with the source.  d_sse: `batch` 8-byte aligned words on
 * the device; d_status[f] (may be NULL): a failure of the front stages.  h_quality as in
 * himg_hip_encode_device_q (a value outside [0, 100]: HIMG_ERR_ARG, nothing launched or written).
 */
int himg_hip_encode_sse_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                               int pixel_stride, int num_channels, const int32_t *h_quality, int use_ycbcr,
                               uint64_t *d_sse, int32_t *d_status, void *stream);
/*
 * Encode to a distortion target: "at least this good, in as few bytes as the search finds".  Per
 * frame, frames independent of each other; T its target (h_max_sse: a HOST array of `batch` values,
 * staged like h_budgets):
 *   1. probe qmax.  sse(qmax) > T: the frame fails -- d_quality[f] = -1, d_sizes[f] = 0, d_status[f] =
 *      HIMG_ERR_TARGET, d_sse[f] = sse(qmax); its bytes in d_out are unspecified but stay inside its
 *      out_stride bytes.  The other frames go on.
 *   2. if qmin < qmax, probe qmin.  It meets T: the result is qmin.
 *   3. otherwise lo = qmin, hi = qmax; while hi - lo > 1: mid = (lo + hi) >> 1; sse(mid) <= T ?
 *      hi = mid : lo = mid.  The result is hi.
 * Every frame with a result is then encoded at it (byte-identical to himg_hip_encode at that
 * quality); d_sse[f] holds sse at the result -- exact, so d_sse[f] <= T.
 * sse is NOT monotone in the quality: eight small test pictures have between 4 and 39 places in
 * 0 .. 99 where sse(q + 1) > sse(q), and random noise (64 x 64 RGBA, YCbCr) has its minimum 47 717 at
 * q = 86 and 66 146 at q = 100 (tests/test_target_host.py holds the oracle to both).  So this is THE
 * SEARCH'S result, a deterministic quality that meets the target -- not the least such quality, and
 * a target that some quality below qmax would meet fails when qmax itself does not.
 * Asynchronous, no host synchronisation: himg_hip_budget_probes(qmin, qmax) probes for every frame.
 * Argument checks as himg_hip_encode_budget_device.
 */
int himg_hip_encode_target_device(himg_hip_ctx *ctx, const void *d_frames, int batch, int width, int height,
                                  int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                                  const uint64_t *h_max_sse, void *d_out, size_t out_stride, uint32_t *d_sizes,
                                  int32_t *d_quality, uint64_t *d_sse, int32_t *d_status, void *stream);
/* The host forms, as himg_hip_encode_budget_to / _batch: *quality / qualities[i] = -1 and the error
 * HIMG_ERR_TARGET for a frame that misses its target at qmax; *sse / sses[i]: the sse reached. */
int himg_hip_encode_target_to(himg_hip_ctx *ctx, const uint8_t *data, int width, int height,
                              int pixel_stride, int num_channels, int qmin, int qmax, int use_ycbcr,
                              uint64_t max_sse, uint8_t *dst, size_t dst_cap, size_t *out_size, int *quality,
                              uint64_t *sse);
int himg_hip_encode_target_batch(himg_hip_ctx *ctx, const uint8_t *const *frames, int n, int width,
                                 int height, int pixel_stride, int num_channels, int qmin, int qmax,
                                 int use_ycbcr, const uint64_t *max_sse, uint8_t *const *dst,
                                 const size_t *dst_cap, size_t *out_sizes, int *qualities, uint64_t *sses);
/* Host only, no GPU: the largest sse with which a W x H x C picture still has at least psnr_db dB,
 * floor(255^2 W H C / 10^(dB / 10)) in double arithmetic.  HIMG_ERR_ARG for a non-finite or negative
 * dB or a bad geometry; a dB so high that the result is 0 asks for a lossless result. */
int himg_hip_psnr_to_sse(double psnr_db, int width, int height, int num_channels, uint64_t *max_sse);

/* ---- 1/8-scale preview: the low-res picture at the front of the stream ------ */
/*
 * The LRES chunk holds one sample per 8x8 block and channel and comes
 * before QCFG, FMAP and FRES.  A preview is that plane as a picture: ceil(H/8) rows x
 * ceil(W/8) columns x C channels, interleaved u8, tightly packed, rows and channels in the
 * order of the full decode's output; pixel (u, v) is the decoder's low-res sample of block
 * (u, v) (downsampled.cpp:318-382), through the colour inverse YCbCr::YCbCrToRGB
 * (ycbcr.cpp:54-82) on channels 0..2 when FRMT's colour space is 1 and C >= 3.  A sample is
 * the box over pixels 8u-3 .. 8u+4 (downsampled.cpp:67-114): the thumbnail sits 3 pixels up and
 * left of the block grid.  No further filtering.
 * Verdict: exactly the reference decoder's first four stages (decoder.cpp:95-118: RIFF
 * including file_size + 8 == packed_size, FRMT, LMAP, LRES with the deviations listed at
 * HIMG_OPT_FIX_T2, which applies to the LRES stream as in the full decode); damage in QCFG,
 * FMAP or FRES is not seen.  HIMG_ERR_FORMAT and himg_hip_last_error as himg_hip_decode
 * for those stages.
 * Bytes read: nothing at or beyond head_bytes (the end of the LRES chunk) rounded up to the
 * next multiple of 4 -- the LRES readers work on whole dwords and are bounded there.  So a
 * caller may preview a file of which only the first head_bytes bytes are present;
 * packed_size stays the size of the whole stream (the RIFF check needs it).
 */
/* Host only, no GPU: the checks of stages 1-3 and the chunk walk to the end of LRES
 * (decoder.cpp:144-212 and the forward search of :428-461, skipping unknown chunks), on the
 * `avail` bytes present at `packed` (nothing at or beyond avail is read).  *pw / *ph / *channels:
 * the preview's geometry; *head_bytes: where the LRES chunk ends.  HIMG_ERR_FORMAT where the
 * reference rejects the head (stages 1-3, or no LRES chunk); HIMG_ERR_CAPACITY when avail ends
 * before the end of LRES (*head_bytes then set if the LRES header was reached, else 0);
 * HIMG_ERR_UNSUPPORTED as himg_hip_peek. */
int himg_hip_preview_peek(const uint8_t *packed, size_t avail, size_t packed_size, int *pw, int *ph,
                          int *channels, size_t *head_bytes);
/* The preview into caller-owned host memory; the capacity protocol of himg_hip_decode_to
 * (HIMG_ERR_CAPACITY with the geometry set; himg_hip_fetch_last copies the result).  `packed`
 * holds at least head_bytes bytes; only those are read and uploaded. */
int himg_hip_preview_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, uint8_t *dst,
                        size_t dst_cap, int *pw, int *ph, int *channels);
/* n streams, the semantics of himg_hip_decode_batch: geometry per frame from FRMT, a frame that
 * fails (or whose dst is too small) gets pw[i] = 0 and does not stop the others, the return
 * value is the first error.  Frames that share a geometry go through one device launch
 * of up to 256 frames; more such frames take several launches. */
int himg_hip_preview_batch(himg_hip_ctx *ctx, const uint8_t *const *packed, const size_t *packed_sizes,
                           int n, uint8_t *const *dst, const size_t *dst_cap, int *pw, int *ph,
                           int *channels);
/* The contract of himg_hip_decode_device (the geometry validated on the device against each
 * stream's FRMT chunk, as there), except that d_out holds
 * batch x ceil(H/8) x ceil(W/8) x C bytes and each stream is read only up to its head_bytes
 * rounded up to 4. */
int himg_hip_preview_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                            const uint32_t *h_sizes, int batch, int width, int height,
                            int num_channels, void *d_out, int32_t *d_status, void *stream);

/* ---- region decode: rectangles at full resolution ------------------------------ */
/*
 * A rectangle R = (x, y, w, h) with w, h >= 1, x, y >= 0, x + w <= W and y + h <= H (any other
 * rectangle: HIMG_ERR_ARG).  R touches block rows r0 = y / 8 .. r1 = ceil((y + h) / 8) and tile
 * columns x / 8 .. ceil((x + w) / 8).  Output: h rows x w columns x C channels, interleaved u8,
 * tightly packed; pixel (i, j) is byte for byte pixel (y + i, x + j) of himg_hip_decode's output,
 * under the same HIMG_OPT_FIX_T2 setting.
 * Verdict: HIMG_ERR_FORMAT, with himg_hip_decode's himg_hip_last_error wording, wherever the
 * reference fails in the container stages (RIFF .. FMAP), the FRES chunk and its tree, the size
 * headers of rows 0 .. r1-1, or the entropy decode of rows r0 .. r1-1 with each row's
 * end-of-block checks.  Damage elsewhere -- row headers from r1 on, payloads of rows outside
 * [r0, r1) -- is not seen; when r1 is the last block row the headers are walked to the end of
 * the chunk, so that a whole-frame rectangle gets himg_hip_decode's verdict for every stream.
 * Bytes used: [0, head_bytes) (container, LRES, QCFG, FMAP, the FRES tree), the size header of
 * each row 0 .. r1-1 and the payloads of rows r0 .. r1-1.  Nothing else decides the pixels or the
 * verdict.  The kernels do load a little more and ignore it: whole dwords around these bytes, the
 * first 384 bytes of the FRES chunk (the tree is staged in one piece, which may reach into the
 * first rows), and a few dwords behind a row's payload (the bit readers' look-ahead).  Every load
 * stays inside the stream.
 */
typedef struct himg_hip_region_plan {
  int width, height, num_channels;   /* the frame's geometry (FRMT) */
  int row0, row1;                    /* touched block rows [row0, row1) */
  size_t head_bytes;                 /* where the first row header starts (rows_first) */
  size_t rows_begin, rows_end;       /* bytes of rows row0 .. row1-1 with their size headers */
} himg_hip_region_plan;
/* Host only, no GPU: validates R against FRMT and walks the row headers up to row1 only (a
 * bounded himg_hip_index_host; error codes as there: HIMG_ERR_FORMAT for a container, tree or
 * header the decoder rejects, HIMG_ERR_UNSUPPORTED as himg_hip_peek, HIMG_ERR_ARG for a bad
 * rectangle).  himg_hip_decode_region_to indexes on the host and uploads [0, head_bytes) and
 * [rows_begin, rows_end), each at its offset in the stream; a caller of
 * himg_hip_decode_region_device provides the size headers of rows 0 .. row0-1 as well (the device
 * walks them).  Other bytes of the buffer may hold anything. */
int himg_hip_region_peek(const uint8_t *packed, size_t packed_size, int fix_t2, int x, int y, int w, int h,
                         himg_hip_region_plan *plan);
/* R of one host stream into caller-owned host memory; the capacity protocol of himg_hip_decode_to
 * (HIMG_ERR_CAPACITY with *width = w, *height = h, *channels = C set; himg_hip_fetch_last copies
 * the resident result).  Only the two ranges of the plan are uploaded. */
int himg_hip_decode_region_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int x, int y,
                              int w, int h, uint8_t *dst, size_t dst_cap, int *width, int *height,
                              int *channels);
/* R of every stream of a batch in HBM (the same R in every frame; himg_hip_decode_regions_device
 * below takes an origin per frame): the argument and alignment
 * contract of himg_hip_decode_device, except that d_out holds batch x h x w x C bytes, frame f at
 * f * h * w * C (no alignment asked of a frame's start), and only the bytes used (above) of each
 * stream decide the result. */
int himg_hip_decode_region_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                  const uint32_t *h_sizes, int batch, int width, int height,
                                  int num_channels, int x, int y, int w, int h, void *d_out,
                                  int32_t *d_status, void *stream);
/* The window w x h at origin (x_f, y_f) = h_origins[2f], h_origins[2f+1] in frame f of a batch in
 * HBM: himg_hip_decode_region_device with a rectangle per frame.  h_origins is a HOST array of
 * 2 x batch values, like h_sizes; it reaches the device with the sizes (no host synchronisation).
 * Every rectangle is checked on the host before anything is launched: one outside its frame makes
 * the call return HIMG_ERR_ARG and nothing is written (neither d_out nor d_status).  d_out holds
 * batch x h x w x C bytes, frame f at f * h * w * C.  Grid limits: batch <= 65535,
 * batch x C <= 65535, block rows + 1 <= 65535.  Frame f's verdict and bytes used are exactly those
 * of its own rectangle alone (above): damage its rectangle does not look at, or damage in another
 * frame, changes neither its status nor its pixels. */
int himg_hip_decode_regions_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                   const uint32_t *h_sizes, int batch, int width, int height,
                                   int num_channels, const int32_t *h_origins, int w, int h,
                                   void *d_out, int32_t *d_status, void *stream);
/* n host streams, rectangle i = rects[4i .. 4i+3] = {x, y, w, h}; any geometry and window size
 * per frame.  Frame i's output goes to dst[i] (capacity dst_cap[i] >= w x h x C) and its
 * widths / heights / channels are set on success.  A frame that fails -- a NULL or bad stream, an
 * unsupported geometry, a bad rectangle (HIMG_ERR_ARG), a NULL or too-small dst
 * (HIMG_ERR_CAPACITY), or the decode's verdict -- gets widths[i] = heights[i] = channels[i] = 0;
 * the other frames go on, and the call returns the first such error.  Frame i's status is the one
 * himg_hip_decode_region_to gives for its rectangle alone.  Each frame is planned on the host
 * (himg_hip_region_peek, under the context's HIMG_OPT_FIX_T2) and only its [0, head_bytes) and
 * [rows_begin, rows_end) are uploaded, with the host's row index.  Frames that share
 * (W, H, C, w, h) go through one device launch, in the order of their first frame, of at most 256
 * frames whose streams -- each taking the launch's largest stream size in the staging buffer --
 * fit in 1 GiB (one frame at least).  A stream the host cannot plan (or of one block row) goes
 * through himg_hip_decode_region_to's own path, uploaded whole. */
int himg_hip_decode_regions_batch(himg_hip_ctx *ctx, const uint8_t *const *packed,
                                  const size_t *packed_sizes, int n, const int32_t *rects,
                                  uint8_t *const *dst, const size_t *dst_cap,
                                  int *widths, int *heights, int *channels);

/* ---- region decode: many windows of one stream ----------------------------------- */
/*
 * The region entry points above take one window per stream.  These take a window -> stream map, the
 * stream-side counterpart of frame_pitch = 0 in himg_hip_src / himg_hip_dst ("all windows in ONE
 * picture"): a tile or viewport server over one very large picture, detection crops, several random
 * crops per image.  The head of a stream -- the container parse, the LRES chain for the low-res plane,
 * the walk over the row headers -- runs ONCE per stream however many windows name it, and a block row
 * that several windows touch is counted once.
 *
 * Window k is the w x h rectangle at (x_k, y_k) = h_origins[2k], h_origins[2k+1] of stream
 * s_k = h_stream_of[k]; its pixels go to d_out + k * h * w * C, tightly packed, and its verdict to
 * d_status[k].  For every window, bytes and status are EXACTLY what himg_hip_decode_regions_device
 * gives for that stream as a frame of its own with that rectangle alone, under the same
 * HIMG_OPT_FIX_T2: the same status word and the same bytes used (the head, the size headers of rows
 * 0 .. r1_k-1, the payloads of rows r0_k .. r1_k-1).
 * Independence: damage that window k's rectangle does not look at changes neither its status nor its
 * pixels -- also when another window of the SAME stream looks at it and fails.  A payload row that is
 * rejected fails only the windows that touch that row.  A size header rejected at row j fails exactly
 * the windows with r1_k > j.  A window with r1_k below the last block row accepts a FRES chunk that
 * ends right behind row r1_k - 1; only windows that reach the last block row take the verdict of the
 * walk to the end of the chunk.  A head verdict (RIFF .. FMAP, the FRES tree, the LRES chain) is every
 * window's of that stream and no other stream's.
 * A failed window's pixels are unspecified but stay inside its own h x w x C bytes; nothing outside
 * n_windows x h x w x C bytes of d_out and n_windows words of d_status is written.  Windows may
 * overlap, repeat and come in any order of stream.  A stream that no window names is allowed: it decides
 * nothing, has no status of its own, and its bytes may be anything (its h_sizes entry still has to fit
 * in_stride).
 * Asynchronous on `stream` like the other device entries; h_stream_of (n_windows values) and h_origins
 * (2 x n_windows) are HOST arrays that reach the device with the sizes, with no host synchronisation.
 * Checked on the host before anything is launched -- NULLs, n_streams or n_windows outside 1 .. 65535, the
 * grid limits of himg_hip_decode_regions_device over the streams (n_streams x C <= 65535,
 * block rows + 1 <= 65535), an s_k outside [0, n_streams), a rectangle outside width x height: any of them
 * returns HIMG_ERR_ARG and neither d_out nor d_status is written.
 *
 * Not in this change: scaled, tensor and pitched store forms; a host batch over many streams; the
 * row-sharded and multi-GPU paths; the C++ classes and the command-line tools; keeping a parsed head
 * across calls.
 */
int himg_hip_decode_stream_regions_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                          const uint32_t *h_sizes, int n_streams, int width, int height,
                                          int num_channels, const int32_t *h_stream_of,
                                          const int32_t *h_origins, int n_windows, int w, int h, void *d_out,
                                          int32_t *d_status, void *stream);
/* Host only, no GPU: per window its himg_hip_region_plan, and the merged, sorted byte ranges a caller
 * must have present: [0, head_bytes) and the union of the windows' [rows_begin, rows_end), as
 * ranges[2i] .. ranges[2i+1], *n_ranges of them; ranges holds up to 2 * (n + 1) values.  Codes as
 * himg_hip_region_peek (a bad rectangle: HIMG_ERR_ARG); the call returns the first window's that is not
 * HIMG_OK.  A window without a plan contributes no range; its plan has row1 = 0, row0 = its code and no
 * bytes -- a header chain that breaks at row j leaves the windows with r1 <= j their plans. */
int himg_hip_stream_regions_peek(const uint8_t *packed, size_t packed_size, int fix_t2, int n,
                                 const int32_t *origins, int w, int h, himg_hip_region_plan *plans,
                                 size_t *ranges, int *n_ranges);
/* One HOST stream, n windows of w x h into dst (n x h x w x C bytes, window k at k * h * w * C);
 * statuses[k]: HIMG_OK or window k's error; returns the first error (himg_hip_last_error words it).  A bad
 * rectangle fails the call (HIMG_ERR_ARG) before anything runs.  The capacity protocol of
 * himg_hip_decode_region_to: HIMG_ERR_CAPACITY with *width = w, *height = h, *channels = C and the
 * statuses set, and himg_hip_fetch_last copies the resident n x h x w x C bytes.  The host plans the
 * windows and uploads only the merged ranges of himg_hip_stream_regions_peek with its row index; a
 * stream it cannot index for every window goes up whole and takes the device walk. */
int himg_hip_decode_stream_regions_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int n,
                                      const int32_t *origins, int w, int h, uint8_t *dst, size_t dst_cap,
                                      int *statuses, int *width, int *height, int *channels);

/* ---- region decode: streams opened once, windows in many calls -------------------- */
/*
 * himg_hip_decode_stream_regions_device makes ONE call with many windows cheap; a tile server, a viewer
 * that pans or a loader that draws crops over an epoch makes MANY calls on the same streams, and each of
 * them ran the whole head again.  An opened-streams handle keeps what the head produces -- the parsed
 * frame, the FRES tables, the row index, the low-res plane -- and the per-row records of the count
 * kernels in device memory of its own:
 *   open     runs the head once per stream and walks ALL row headers once;
 *   a call   decodes windows against the handle.  No parse, no LRES chain, no walk; a block row is counted
 *            the first time any call touches it and never again.
 *
 * Nothing new is defined about pixels or verdicts.  For any sequence of himg_hip_opened_regions_device
 * calls on a handle -- w x h may differ from call to call; windows may overlap, repeat and come in any
 * order of stream -- each call's d_status words, and the pixels of every window with status 0, are EXACTLY
 * what himg_hip_decode_stream_regions_device gives for the same streams, map, origins and w x h under the
 * HIMG_OPT_FIX_T2 the context had at open (the handle records it; a later change of the option does not
 * reach the handle).  Its independence rules hold in whichever call a window comes, and so do its argument
 * checks (HIMG_ERR_ARG, nothing written, no row marked as counted), its grid limits and the rule that
 * nothing outside n_windows x h x w x C bytes of d_out and n_windows words of d_status is written.
 *
 * Bytes used.  Open loads [0, head_bytes) and the size headers to the end of the FRES chunk.  After open
 * the device form loads only payload bytes of touched rows from d_packed (with the bit readers' look-ahead):
 * the head and the size headers are never read again.  The caller keeps d_packed valid and its payloads
 * unchanged while the handle lives; the host form uploads the stream into memory the handle owns.
 *
 * Ownership and order.  A handle belongs to the context that opened it; with another context, or after
 * himg_hip_close_streams, every entry returns HIMG_ERR_ARG.  It is ordered by the caller's stream alone,
 * under the rule of "Streams" above: open and the calls queued behind it on one stream need no host wait.
 * Open may wait for the device once, when it allocates the handle's memory (the rule of a context's first
 * call at a larger geometry); nothing else synchronises.  himg_hip_close_streams waits for the handle's
 * last call and frees; himg_hip_destroy closes the handles that are left.  A stream whose head fails still
 * opens: its windows get that status.
 *
 * Device memory of a handle over n streams, each term rounded up to 256 bytes (himg_hip_opened_bytes;
 * rows = ceil(H / 8), cols = ceil(W / 8)):
 *   n x 1616                                        the parsed frames
 *   n x 4176 + n x 32768 + n x 16384 + n x 16384    the tables (nodes, groups, count groups, second level)
 *   n x rows x 8                                    the row index
 *   n x roundup256(C x rows x cols)                 the low-res planes
 *   n x rows x (2 x 1024 + 72) x 4                  the records
 *   (n x (rows + 1) x 8 + n x 4 + n x rows x 8) x 4 the kernels' diagnostics
 *   n x 12                                          the packed sizes and the walk's words
 * The records (8480 bytes per block row) and the low-res planes dominate: 17.4 + 16.8 MB for one 16384^2
 * RGBA stream, 704 MB for 128 x 4096^2.
 *
 * Scaled windows (himg_hip_opened_scaled_regions_device / _to): a viewer that pans also zooms, and a tile
 * server serves every pyramid level.  scale_log2 is 1, 2 or 3 (anything else: HIMG_ERR_ARG); window k is the
 * w x h rectangle at (x_k, y_k) IN THE COORDINATES OF STREAM stream_of[k]'s PICTURE AT THAT SCALE -- ow x oh by
 * himg_hip_scaled_size at scales 1 and 2, ceil(W / 8) x ceil(H / 8) at scale 3 --, and must lie inside it.  The
 * output is n_windows x h x w x C interleaved bytes, window k at k h w C.  Every check and rule of
 * himg_hip_opened_regions_device above holds: all arguments are checked on the host before anything is
 * launched, a refusal writes nothing and marks no row as counted, the call is asynchronous on the caller's
 * stream, nothing outside the output bytes and the n_windows status words is written, and the
 * HIMG_OPT_FIX_T2 recorded at open applies.  One scale per call.
 *   scales 1, 2   d_status[k], and the bytes of every window with status 0, are exactly those of
 *                 himg_hip_decode_scaled_regions_device on stream s_k alone (batch 1) with that origin, w x h
 *                 and scale: the verdict is the region decode's of the covered full-resolution rectangle R^
 *                 (see the scaled region decode), so a whole-picture window gets himg_hip_decode's.  The
 *                 independence rules hold across scales as across calls: a window that meets damage fails
 *                 alone, in whichever call and at whichever scale it comes, and no call changes what a later
 *                 call returns, at this scale, another, or full resolution.  The window touches block rows
 *                 [y / S, ceil((y + h) / S)), S = 8 >> scale_log2 -- R^'s rows.  The records are shared: a
 *                 block row counted by a full-resolution call serves a scaled call and the other way round,
 *                 so a row is counted once per handle whatever mix of entry points touches it, and
 *                 rows_counted (himg_hip_opened_info) counts these rows like any others.
 *   scale 3       d_status[k] is stream s_k's head verdict, the word open wrote to d_head_status; where it
 *                 is 0 the bytes are the crop of himg_hip_preview_device's output for that stream, read
 *                 from the low-res plane the handle holds.  No row is touched: no count runs, rows_counted
 *                 does not move, and d_packed is not read at all.
 *
 * Not in this change: tensor and pitched store forms; mixed scales within one call; a stateless many-windows
 * scaled decode; eviction or a cap on a handle's memory; re-opening on a changed stream; a prefix that grows under a handle; the C++ classes and the
 * command-line tools; the multi-GPU handle and the row-sharded paths.
 */
typedef struct himg_hip_opened himg_hip_opened;

/* Host only, no GPU: the device bytes a handle over n_streams streams of this geometry holds, without the
 * streams.  HIMG_ERR_ARG: a bad geometry, n_streams outside 1 .. 65535, bytes NULL. */
int himg_hip_opened_bytes(int width, int height, int num_channels, int n_streams, size_t *bytes);

/* Streams in HBM: the argument contract of himg_hip_decode_stream_regions_device up to num_channels.
 * d_head_status (may be NULL): n_streams words, each stream's head verdict. */
int himg_hip_open_streams_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, const uint32_t *h_sizes,
                                 int n_streams, int width, int height, int num_channels,
                                 int32_t *d_head_status, himg_hip_opened **out, void *stream);
/* One HOST stream, uploaded whole into memory the handle owns; the geometry from FRMT.  The rows are
 * indexed on the host where it can (himg_hip_index_host); a stream it cannot index takes the device walk.
 * On the null stream; returns when the upload has read `packed`. */
int himg_hip_open_stream_host(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, himg_hip_opened **out);

/* Windows against a handle: h_stream_of, h_origins, n_windows, w, h, d_out, d_status and stream as in
 * himg_hip_decode_stream_regions_device. */
int himg_hip_opened_regions_device(himg_hip_ctx *ctx, himg_hip_opened *o, const int32_t *h_stream_of,
                                   const int32_t *h_origins, int n_windows, int w, int h,
                                   void *d_out, int32_t *d_status, void *stream);
/* The host form: n windows into dst (n x h x w x C bytes), statuses[k] as himg_hip_decode_stream_regions_to;
 * h_stream_of may be NULL (every window of stream 0).  The capacity rule of himg_hip_decode_pyramid_to: a
 * NULL or short dst gives HIMG_ERR_CAPACITY with *width = w, *height = h, *channels = C and nothing
 * decoded.  Waits for its result (on the null stream). */
int himg_hip_opened_regions_to(himg_hip_ctx *ctx, himg_hip_opened *o, int n, const int32_t *h_stream_of,
                               const int32_t *origins, int w, int h, uint8_t *dst, size_t dst_cap,
                               int *statuses, int *width, int *height, int *channels);
/* Scaled windows against a handle (the section above): scale_log2 = 1, 2, 3; the origins and w x h in the
 * picture at that scale; everything else as in himg_hip_opened_regions_device. */
int himg_hip_opened_scaled_regions_device(himg_hip_ctx *ctx, himg_hip_opened *o, int scale_log2,
                                          const int32_t *h_stream_of, const int32_t *h_origins, int n_windows,
                                          int w, int h, void *d_out, int32_t *d_status, void *stream);
/* The host form, with himg_hip_opened_regions_to's contract: a NULL h_stream_of means stream 0; a NULL or short
 * dst gives HIMG_ERR_CAPACITY with *width = w, *height = h, *channels = C, nothing decoded and nothing counted;
 * returns the first error in window order. */
int himg_hip_opened_scaled_regions_to(himg_hip_ctx *ctx, himg_hip_opened *o, int scale_log2, int n,
                                      const int32_t *h_stream_of, const int32_t *origins, int w, int h, uint8_t *dst,
                                      size_t dst_cap, int *statuses, int *width, int *height, int *channels);
/* What a handle holds (any pointer may be NULL); rows_counted: the (stream, block row) pairs a call has
 * queued a count for. */
int himg_hip_opened_info(const himg_hip_opened *o, int *n_streams, int *width, int *height, int *channels,
                         size_t *device_bytes, long long *rows_counted);
void himg_hip_close_streams(himg_hip_ctx *ctx, himg_hip_opened *o);

/* ---- decode into windows of pitched destination pictures ------------------------- */
/*
 * The decode entry points above write batch x H x W x C tightly packed bytes.  These take a row pitch,
 * a pixel stride and an origin per frame, the way himg_hip_encode_windows_device does on the other
 * side: a surface with padded rows (hipMallocPitch), an RGB stream into an RGBA buffer that keeps its
 * alpha, a region pasted into a canvas, or the tile streams of one large picture stitched where they
 * belong (frame_pitch = 0) -- without a second pass that moves every output byte again.
 */
typedef struct himg_hip_dst {
  int width, height;      /* the destination pictures in pixels: every window lies inside */
  int pixel_stride;       /* bytes from a pixel to the next, >= num_channels */
  size_t row_pitch;       /* bytes from a row to the next, >= width * pixel_stride */
  size_t frame_pitch;     /* bytes from destination picture f to f + 1; 0: all windows lie in ONE picture */
} himg_hip_dst;

/* Where the bytes go.  Frame f's decoded picture is W x H (himg_hip_decode_into_device), or the window
 * w x h at (sx_f, sy_f) = h_src_origins[2 f], [2 f + 1] of the decoded picture, under the rectangle
 * rules of himg_hip_decode_regions_device (himg_hip_decode_regions_into_device).  Its pixel (i, j),
 * channel c < C, is written to
 *   d_dst + f * frame_pitch + (y_f + i) * row_pitch + (x_f + j) * pixel_stride + c,
 * (x_f, y_f) = h_origins[2 f], h_origins[2 f + 1] (h_dst_origins), and is byte for byte what
 * himg_hip_decode_device (himg_hip_decode_regions_device) writes for that stream under the same
 * HIMG_OPT_FIX_T2 setting.
 *
 * Nothing else is written: not bytes C .. pixel_stride - 1 of a pixel (an RGB stream decoded into RGBA
 * keeps the alpha that was there), not the row padding, not pixels outside the window, not the gap
 * between pictures, and nothing at or beyond *bytes of himg_hip_dst_extent: the largest
 *   f * frame_pitch + (y_f + h - 1) * row_pitch + (x_f + w) * pixel_stride
 * over the batch -- a buffer may end with its last window's last pixel.  The kernels use a 16-byte or a
 * 4-byte store only where every byte it covers is one of these.
 *
 * Status: frame f's d_status is exactly himg_hip_decode_device's (himg_hip_decode_regions_device's,
 * with that entry's bytes-used rule).  A failed frame's window holds unspecified bytes; nothing outside
 * that window is touched and its neighbours are unaffected.  The calls are asynchronous: the origins
 * are HOST arrays of 2 * batch values that ride to the device with the sizes, the descriptor travels
 * in the kernel arguments.
 *
 * Overlapping windows of different frames in one picture (frame_pitch = 0) are not checked: a byte in
 * an overlap is one of the frames' bytes, which one is unspecified.
 *
 * Checks, all on the host before anything is launched -- a failure returns HIMG_ERR_ARG and neither
 * d_dst nor d_status is written:
 *   - dst NULL, or a picture or window size that is not positive;
 *   - pixel_stride < num_channels;
 *   - row_pitch < width * pixel_stride;
 *   - frame_pitch neither 0 nor at least (height - 1) * row_pitch + width * pixel_stride;
 *   - a window not inside width x height (x_f, y_f >= 0, x_f + w <= width, y_f + h <= height);
 *   - d_dst not 16-byte aligned;
 *   - for pixel_stride == 4: row_pitch or frame_pitch not a multiple of 4.
 * The origins are otherwise unconstrained, odd ones included.  The stream-side arguments are checked
 * as in himg_hip_decode_device / himg_hip_decode_regions_device, whose grid limits apply.
 *
 * Not in this change: pitched forms of the preview, scaled, scaled-region and tensor decodes; a batch
 * host form; the row-sharded and multi-GPU paths; the C++ classes; the command-line tools. */
/* Host only, no GPU: the checks above (those of dst, the window size w x h and the origins;
 * num_channels in 1 .. 4), the same codes, and *bytes. */
int himg_hip_dst_extent(const himg_hip_dst *dst, int num_channels, int batch, const int32_t *h_origins,
                        int w, int h, size_t *bytes);
int himg_hip_decode_into_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                const uint32_t *h_sizes, int batch, int width, int height,
                                int num_channels, void *d_dst, const himg_hip_dst *dst,
                                const int32_t *h_origins, int32_t *d_status, void *stream);
int himg_hip_decode_regions_into_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                        const uint32_t *h_sizes, int batch, int width, int height,
                                        int num_channels, const int32_t *h_src_origins, int w, int h,
                                        void *d_dst, const himg_hip_dst *dst, const int32_t *h_dst_origins,
                                        int32_t *d_status, void *stream);
/* A HOST stream into a HOST picture described by dst (frame_pitch is ignored) at (x, y): decoded on the
 * device as himg_hip_decode_to does, then its rows are copied into the picture at row_pitch and
 * pixel_stride (the same bytes, and nothing else, as above).  The geometry is reported through
 * *width / *height / *channels as soon as the header is read; a picture that does not fit at (x, y), or
 * a descriptor the checks above refuse, returns HIMG_ERR_ARG with dst_data untouched. */
int himg_hip_decode_into_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                            uint8_t *dst_data, const himg_hip_dst *dst, int x, int y, int *width,
                            int *height, int *channels);

/* ---- tensor decode: planar, normalised float output ------------------------------ */
/*
 * The decode in the form a network takes: the first Co channels of the picture (3 of RGBA drops
 * alpha), planar, cast and normalised -- instead of a second pass over the interleaved bytes.
 * Output: [batch][Co][H][W] elements of the chosen type, tightly packed, frame f at element
 * f * Co * H * W.  Element (f, c, i, j) = cvt(fma_f32((float)p, scale[c], bias[c])):
 *   p        byte (i, j, c) of himg_hip_decode's output for that stream, under the same
 *            HIMG_OPT_FIX_T2 setting;
 *   fma_f32  ONE fused multiply-add in binary32, round to nearest even, denormals kept;
 *   cvt      the identity for HIMG_DT_F32; for HIMG_DT_F16 / HIMG_DT_BF16 the conversion of that
 *            binary32 value, round to nearest even (never a round-toward-zero pack).
 * The value is fully determined: results are compared bit for bit, not within a tolerance.
 * Descriptor errors: an unknown dtype, out_channels outside 1 .. C, or a non-finite scale / bias
 * among the first Co -- HIMG_ERR_ARG, nothing launched, neither d_out nor d_status written.
 * Entries of scale / bias from Co on are ignored.  d_out's base must be 16-byte aligned
 * (HIMG_ERR_ARG otherwise); only the base is constrained.
 * Not in this form (they keep their interleaved u8 output): the scaled, scaled-region and preview
 * decodes, the host-memory entry points (_to, _batch), the row-sharded and multi-GPU paths and
 * the command-line tools.  There is no NHWC float layout and no encode from float tensors.
 */
#define HIMG_DT_F32 0
#define HIMG_DT_F16 1
#define HIMG_DT_BF16 2
typedef struct himg_hip_tensor_desc {
  int dtype;            /* HIMG_DT_* */
  int out_channels;     /* Co, 1..C: the first Co channels of the decoded picture (3 of RGBA drops alpha) */
  float scale[4], bias[4];   /* per output channel; entries >= Co are ignored */
} himg_hip_tensor_desc;
/* Host only, no GPU: validates the descriptor against C = num_channels (the rules above) and the
 * geometry, and sets *bytes_per_frame = Co * h * w * element size. */
int himg_hip_tensor_bytes(const himg_hip_tensor_desc *t, int num_channels, int w, int h, size_t *bytes_per_frame);
/* Streams of a batch in HBM: the argument, alignment, asynchrony and verdict contract of
 * himg_hip_decode_device with the output above.  Frame f's status is exactly
 * himg_hip_decode_device's; a failed frame's output is as unspecified as it is there, and its
 * neighbours are unaffected.  The descriptor travels in the kernel arguments: no host
 * synchronisation, no extra copy. */
int himg_hip_decode_tensor_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                  const uint32_t *h_sizes, int batch, int width, int height,
                                  int num_channels, const himg_hip_tensor_desc *t, void *d_out,
                                  int32_t *d_status, void *stream);
/* The window w x h at origin (x_f, y_f) of frame f (a data loader's random crop): the contract of
 * himg_hip_decode_regions_device -- rectangles checked on the host before anything is launched,
 * per-frame verdicts, bytes used, grid limits -- with the output [batch][Co][h][w]: element
 * (f, c, i, j) is the formula above applied to pixel (y_f + i, x_f + j).  Windows are arbitrary:
 * beyond the 16-byte aligned base the stores are only element-aligned, and nothing outside the
 * batch * Co * h * w elements is written. */
int himg_hip_decode_regions_tensor_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                          const uint32_t *h_sizes, int batch, int width, int height,
                                          int num_channels, const int32_t *h_origins, int w, int h,
                                          const himg_hip_tensor_desc *t, void *d_out,
                                          int32_t *d_status, void *stream);

/* ---- planes decode: the stream's own channel planes (luma, alpha, planar YCbCr) ---- */
/*
 * Every other decode ends in the picture BEHIND the colour inverse.  This one stores the stream's own
 * channel planes, the representation the reference decoder holds immediately before YCbCrToRGB
 * (decoder.cpp:372-423): for a colour-space-1 stream of three or four channels plane 0 is the codec's
 * luma, planes 1 and 2 its Cb and Cr, plane 3 alpha.  A greyscale consumer takes plane 0, a compositor
 * plane 3, a video or re-encode pipeline planes 0..2 with no round trip through RGB.  (Luma recomputed
 * from decoded RGB is not the stream's luma: the inverse clamps.)
 *
 * plane_mask has bit c set for each wanted channel c of the stream; it must be non-zero and have no bit
 * at or above num_channels.  P = popcount(plane_mask).  Output: [batch][P][H][W] uint8, tightly packed,
 * the planes in ascending channel order, frame f at f * P * H * W.  Plane c, pixel (y, x) is the byte
 * the reference decoder holds for that channel immediately before YCbCrToRGB: the inverse transform,
 * plus the interpolated low-res plane, clamped to 0..255, dequantised with the chroma shift table
 * exactly where the reference uses it (decoder.cpp:376: channels 1 and 2 of a colour-space-1 stream of
 * three or four channels).  No colour inverse is ever applied.  Where the full decode applies no colour
 * inverse (colour space 0, or C < 3), plane c is channel c of himg_hip_decode_device's output, byte for
 * byte.  What plane 1 means is the stream's business: himg_hip_peek_format reports its colour space.
 * Frame f's status word is exactly himg_hip_decode_device's, under either HIMG_OPT_FIX_T2 setting (the
 * T2 rule included); a failed frame's bytes are unspecified and its neighbours are unaffected.  Only
 * real pixels are stored: nothing is written at or beyond batch * P * H * W.
 * An unselected channel's tiles are not transformed and nothing of it is stored: plane 0 alone of an
 * RGBA stream is a quarter of the output bytes and a quarter of the tile transforms; the entropy
 * decode is the full decode's.
 * Not in this form: the region, scaled, pitched, tensor, prefix, concealing, opened-stream and pyramid
 * decodes, himg::Decoder, the multi-GPU handle and the row-sharded paths; there is no host batch entry.
 */
/* Host only, no GPU: validates num_channels (1..4), plane_mask (the rules above) and the geometry
 * (w, h >= 1, the engine's limits), and sets *bytes_per_frame = P * h * w.  HIMG_ERR_ARG otherwise
 * (also for a NULL result). */
int himg_hip_planes_bytes(int num_channels, uint32_t plane_mask, int w, int h, size_t *bytes_per_frame);
/* Host only, no GPU: himg_hip_peek, and *colour_space = FRMT byte 10 (0: the channels are the picture's
 * own; 1: channels 0..2 of a stream of three or four channels are Y, Cb, Cr). */
int himg_hip_peek_format(const uint8_t *packed, size_t packed_size, int *width, int *height,
                         int *num_channels, int *colour_space);
/* Streams of a batch in HBM: the argument, alignment (d_out's base 16-byte aligned), asynchrony and
 * verdict contract of himg_hip_decode_device with the output above.  A bad mask is HIMG_ERR_ARG:
 * nothing launched, neither d_out nor d_status written.  The mask travels in the kernel arguments: no
 * host synchronisation, no extra copy. */
int himg_hip_decode_planes_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                  const uint32_t *h_sizes, int batch, int width, int height,
                                  int num_channels, uint32_t plane_mask, void *d_out,
                                  int32_t *d_status, void *stream);
/* One stream in host memory, himg_hip_decode_to's rules: the geometry is reported whenever the stream
 * decodes, and with dst == NULL or dst_cap < P * H * W the call returns HIMG_ERR_CAPACITY with
 * width, height and num_channels set (the size to allocate: himg_hip_planes_bytes).  A mask that does
 * not fit the stream's channel count is HIMG_ERR_ARG. */
int himg_hip_decode_planes_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                              uint32_t plane_mask, uint8_t *dst, size_t dst_cap, int *width, int *height,
                              int *num_channels);

/* ---- scaled decode: the picture at 1/2 and 1/4 scale ----------------------------- */
/*
 * scale_log2 = 1 or 2: F = 2^scale_log2 pixels per output sample and side, S = 8 / F coefficients
 * per tile and side.  Output: oh = ceil(H / F) rows x ow = ceil(W / F) columns x C channels,
 * interleaved u8, tightly packed, channels in the order of the full decode.  Tile (u, v)
 * contributes the samples (X, Y), 0 <= X, Y < S, at (S u + X, S v + Y), dropped outside ow x oh.
 * The transform is the sequency-ordered 8-point Walsh-Hadamard (hadamard.cpp:47-103) and the
 * coefficient scan walks square shells (common.cpp:13-22), so the mean of every F x F box of a
 * tile's inverse transform is, in exact arithmetic, the S-point inverse transform of the tile's
 * top-left S x S coefficients -- the first S * S scan positions of each channel.  The decode the
 * format defines at this scale, per tile and channel, with the decoder's own FMAP table and shift
 * table per channel (decoder.cpp:376):
 *   1. d[j][i] = (int16)(unmap(sym) << shift[8 j + i]) for 0 <= i, j < S (quantize.cpp:153-165
 *      restricted to the top-left S x S, the int16 wrap included);
 *   2. rows, then columns: t = (int16)((sum_i d[j][i] w_i(X)) >> 3), p = (int16)((sum_j t[j][X]
 *      w_j(Y)) >> 3), w the S-point sequency-ordered Walsh matrix (S = 4: ++++, ++--, +--+, +-+-;
 *      S = 2: ++, +-): hadamard.cpp:47-74 with its inputs S.. zero and every F-th output;
 *   3. L[Y][X] = (the sum of the F x F box of the tile's interpolated low-res block
 *      (downsampled.cpp:116-169) + F F / 2) >> (2 scale_log2);
 *   4. sample = clamp8((int16)(p + L)) (decoder.cpp:36-75), then YCbCr::YCbCrToRGB
 *      (ycbcr.cpp:54-82) per output pixel where FRMT's colour space is 1 and C >= 3.
 * This is NOT the box-downsample of himg_hip_decode's bytes: the roundings and the clamp come in a
 * different order.  How close the two are is measured in tests/test_scaled_host.py
 * (profiles/scaled_closeness.json).
 * Verdict: exactly himg_hip_decode's, for every stream, under either HIMG_OPT_FIX_T2 setting, with
 * the same himg_hip_last_error wording (decoder.cpp:95-135,298-426): the whole stream is looked at.
 */
/* Host only, no GPU.  HIMG_ERR_ARG for a scale other than 1 or 2 or a non-positive size. */
int himg_hip_scaled_size(int width, int height, int scale_log2, int *ow, int *oh);
/* Streams of a batch in HBM: the argument and alignment contract of himg_hip_decode_device, except
 * that d_out holds batch x oh x ow x C bytes, frame f at f * oh * ow * C (no alignment asked of a
 * frame's start).  Asynchronous, no host synchronisation.  Stands in for Decoder::Decode
 * (decoder.cpp:95-135) followed by a shrink. */
int himg_hip_decode_scaled_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                  const uint32_t *h_sizes, int batch, int width, int height,
                                  int num_channels, int scale_log2, void *d_out, int32_t *d_status,
                                  void *stream);
/* One host stream into caller-owned host memory; the capacity protocol of himg_hip_decode_to
 * (HIMG_ERR_CAPACITY with *width = ow, *height = oh, *channels = C set; himg_hip_fetch_last copies
 * the resident result).  The row index comes from the host (himg_hip_index_host's walk) where the
 * host can build it, as in himg_hip_decode_to. */
int himg_hip_decode_scaled_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, int scale_log2,
                              uint8_t *dst, size_t dst_cap, int *width, int *height, int *channels);
/* n host streams, the semantics of himg_hip_decode_batch: geometry per frame from FRMT, a frame
 * that fails (or whose dst is NULL or too small) gets widths[i] = 0 and does not stop the others,
 * the return value is the first error.  Frames that share a geometry go through one device launch
 * of up to 256 frames whose streams fit 1 GiB of staging; more take several launches. */
int himg_hip_decode_scaled_batch(himg_hip_ctx *ctx, const uint8_t *const *packed, const size_t *packed_sizes,
                                 int n, int scale_log2, uint8_t *const *dst, const size_t *dst_cap,
                                 int *widths, int *heights, int *channels);

/* ---- scaled region decode: rectangles of the picture at 1/2 and 1/4 scale ---------- */
/*
 * scale_log2 = 1 or 2 (any other scale: HIMG_ERR_ARG), F = 2^scale_log2, S = 8 / F, ow = ceil(W / F),
 * oh = ceil(H / F) as in himg_hip_scaled_size.  A rectangle R = (x, y, w, h) IN THE COORDINATES OF THE
 * SCALED PICTURE, with w, h >= 1, x, y >= 0, x + w <= ow and y + h <= oh (any other rectangle:
 * HIMG_ERR_ARG).  Output: h rows x w columns x C channels, interleaved u8, tightly packed; sample
 * (i, j) is byte for byte sample (y + i, x + j) of himg_hip_decode_scaled_*'s output for the same
 * stream, scale and HIMG_OPT_FIX_T2 setting.  No arithmetic of its own: the four steps of the scaled
 * section above are the definition.
 * R touches block rows r0 = y / S .. r1 = ceil((y + h) / S) and tile columns x / S ..
 * ceil((x + w) / S): the rows and columns of the full-resolution rectangle it covers,
 *   R^ = (F x, F y, min(F w, W - F x), min(F h, H - F y)).
 * Verdict and bytes used: exactly those of the region decode of R^ (the region section above) --
 * container stages, FRES chunk and tree, the size headers of rows 0 .. r1-1 (to the end of the chunk
 * when r1 is the last row), the entropy decode of rows r0 .. r1-1 with each row's end-of-block checks;
 * the same code and the same himg_hip_last_error wording.  A whole-picture rectangle therefore gets
 * himg_hip_decode's verdict.  Every load stays inside the stream.
 */
/* Host only, no GPU: validates R against FRMT and fills the plan; it equals himg_hip_region_peek
 * of R^ (a bounded himg_hip_index_host, error codes as there). */
int himg_hip_scaled_region_peek(const uint8_t *packed, size_t packed_size, int fix_t2, int scale_log2, int x,
                                int y, int w, int h, himg_hip_region_plan *plan);
/* R of one host stream into caller-owned host memory: himg_hip_decode_region_to at a scale.  The host
 * indexes; only [0, head_bytes) and [rows_begin, rows_end) of the plan are uploaded; the capacity
 * protocol of himg_hip_decode_to (HIMG_ERR_CAPACITY with *width = w, *height = h, *channels = C set;
 * himg_hip_fetch_last copies the resident result).  Stands in for Decoder::Decode
 * (decoder.cpp:95-135) followed by a shrink and a crop. */
int himg_hip_decode_scaled_region_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                                     int scale_log2, int x, int y, int w, int h, uint8_t *dst, size_t dst_cap,
                                     int *width, int *height, int *channels);
/* The window w x h at origin (x_f, y_f) = h_origins[2f], h_origins[2f+1] of frame f's scaled picture,
 * streams of a batch in HBM: himg_hip_decode_regions_device at a scale, with its contract --
 * h_origins a HOST array of 2 x batch values riding behind the sizes, every rectangle checked on the
 * host before anything is launched (one outside its frame's ow x oh: HIMG_ERR_ARG, neither d_out nor
 * d_status written), d_out = batch x h x w x C bytes, frame f at f * h * w * C with no alignment
 * asked of a frame's start, asynchronous, the same grid limits.  One shared origin is the caller
 * repeating it. */
int himg_hip_decode_scaled_regions_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                          const uint32_t *h_sizes, int batch, int width, int height,
                                          int num_channels, int scale_log2, const int32_t *h_origins, int w,
                                          int h, void *d_out, int32_t *d_status, void *stream);
/* n host streams at one scale, rectangle i = rects[4i .. 4i+3] = {x, y, w, h} of frame i's scaled
 * picture: the contract of himg_hip_decode_regions_batch (a failing frame gets widths[i] =
 * heights[i] = channels[i] = 0 and does not stop the others, the first error is returned; frames
 * that share (W, H, C, w, h) go through launches of at most 256 frames and 1 GiB of staging; only
 * the planned bytes are uploaded; a stream the host cannot plan goes through
 * himg_hip_decode_scaled_region_to's own path). */
int himg_hip_decode_scaled_regions_batch(himg_hip_ctx *ctx, const uint8_t *const *packed,
                                         const size_t *packed_sizes, int n, int scale_log2,
                                         const int32_t *rects, uint8_t *const *dst, const size_t *dst_cap,
                                         int *widths, int *heights, int *channels);

/* ---- picture pyramid: full, 1/2, 1/4 and 1/8 scale in one pass --------------------- */
/*
 * Level k, 0 <= k <= 3, is the picture at 1 / 2^k: oh = ceil(H / 2^k) rows x ow = ceil(W / 2^k)
 * columns x C channels, interleaved u8, tightly packed.  Nothing new is defined:
 *   level 0 is byte for byte himg_hip_decode_device's output,
 *   level 1 and level 2 himg_hip_decode_scaled_device's with scale_log2 = 1 and 2 (the four steps of
 *   the scaled section above),
 *   level 3 himg_hip_preview_device's,
 * for the same stream under either HIMG_OPT_FIX_T2 setting.  What the pyramid saves is the front of
 * the decode -- container parse, LRES chain, row-header walk, row counts and the entropy walk of
 * every block row -- which runs once for all the wanted levels instead of once per entry point; the
 * smaller levels are computed from the row's symbols where the full-resolution store has them.
 * Verdict: ONE per frame, exactly himg_hip_decode's, for every stream, whichever levels are wanted:
 * the whole stream is looked at.  (Level 3 alone is therefore not himg_hip_preview_device, which
 * does not see damage behind LRES and reads only the head of the stream.)  A failed frame's bytes
 * are unspecified at every level; its neighbours are unaffected.
 */
typedef struct himg_hip_pyramid {
  void *level[4];   /* level[k]: batch x ceil(H/2^k) x ceil(W/2^k) x C bytes, frame f at f*oh*ow*C; NULL = not wanted */
} himg_hip_pyramid;
/* Host only, no GPU: level k's size.  Levels 1 and 2: himg_hip_scaled_size; level 3: the preview's
 * geometry, (ceil(W / 8), ceil(H / 8)); level 0: (W, H).  HIMG_ERR_ARG for a level outside 0..3 or a
 * non-positive size. */
int himg_hip_pyramid_size(int width, int height, int level, int *ow, int *oh);
/* Streams of a batch in HBM: the argument, alignment and grid contract of himg_hip_decode_device,
 * with out->level[k] where d_out stands there.  Any non-empty subset of the levels is valid; an empty
 * one, or a NULL `out`, is HIMG_ERR_ARG with nothing launched and nothing written.  Every wanted
 * level's base is 16-byte aligned, as d_out is for the level's own entry point; no alignment is asked
 * of a frame's start.  No byte outside a wanted level's batch * oh * ow * C bytes is written, and
 * nothing at all for a level that is not wanted.  The pointers ride in the kernel arguments, as the
 * tensor and pitched descriptors do: asynchronous, no host synchronisation, `out` itself is not read
 * after the call returns.  d_status[f]: the one verdict of frame f. */
int himg_hip_decode_pyramid_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                   const uint32_t *h_sizes, int batch, int width, int height,
                                   int num_channels, const himg_hip_pyramid *out, int32_t *d_status,
                                   void *stream);
/* One host stream into caller-owned host memory: one upload, one device pass, one download per
 * wanted level.  Level k is wanted when dst[k] is not NULL or dst_cap[k] is not 0; no level wanted:
 * HIMG_ERR_ARG.  A wanted level whose dst is NULL or whose dst_cap is below its oh * ow * C bytes:
 * HIMG_ERR_CAPACITY with *width, *height, *channels (the full picture's) set and nothing decoded;
 * the caller sizes its buffers from himg_hip_peek and himg_hip_pyramid_size.  Nothing is kept
 * resident: this entry point has NO himg_hip_fetch_last protocol (a fetch behind it finds no result). */
int himg_hip_decode_pyramid_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size,
                               uint8_t *const dst[4], const size_t dst_cap[4], int *width, int *height,
                               int *channels);

/* ---- decode a stream prefix: whole block rows exact, the rest from the low-res plane ---- */
/*
 * The format is progressive in file order: the whole low-res plane (LRES)
 * comes first, then QCFG, FMAP and the FRES tree, then the block rows top to bottom, each an
 * independently coded unit behind its own size header.  A prefix is the first `avail` bytes of a stream
 * whose RIFF header declares T = file_size + 8 bytes, 0 <= avail <= T (avail > T: HIMG_ERR_FORMAT).
 * These entry points give the picture as far as it has arrived, at full size.
 *
 * Verdict.  The stages are himg_hip_decode's, under the same HIMG_OPT_FIX_T2.
 *   - RIFF, FRMT, LMAP, LRES, QCFG, FMAP, the FRES chunk header and its tree run exactly as in the full
 *     decode with T where packed_size stands there: chunk bounds are checked against T.
 *   - head_bytes is the offset of the first row header, as in himg_hip_region_plan.  A prefix that ends
 *     before it gives HIMG_ERR_CAPACITY and nothing is decoded.  (A check that fails on bytes below
 *     avail gives HIMG_ERR_FORMAT even then -- unless a chunk found in front of it is not whole below
 *     avail: the decoder reports the first failure in its order of checks, and that chunk may hold one.)
 *   - The row headers are walked by the decoder's rules (huffman_dec.cpp:232-248) for as long as a
 *     header lies wholly below avail.  A wholly present header the decoder rejects: HIMG_ERR_FORMAT.
 *     The first row whose header or payload is not wholly below avail ends the walk without a verdict;
 *     its index is k, the number of complete rows.  A frame of one block row has no header (under
 *     HIMG_OPT_FIX_T2): k = 1 when the FRES chunk ends at or below avail.
 *   - What the decoder judges at the end of the chunk is judged where bytes below avail decide it: a
 *     chunk that ends inside the prefix with fewer blocks than block rows, a header that would cross
 *     the end of the chunk.
 *   - Rows 0 .. k-1 go through the entropy decode with the reference's end-of-block checks; a failure
 *     there is HIMG_ERR_FORMAT.
 *   - Nothing at or beyond avail decides the verdict or a pixel.
 *   - avail == T is himg_hip_decode: the same verdict, the same himg_hip_last_error wording, the same
 *     bytes.
 * Pixels.  H x W x C interleaved u8, laid out as himg_hip_decode's.  The pixel rows of block rows
 * 0 .. k-1 are byte for byte the full decode's.  Those of block rows k .. rows-1 are what the full
 * decode writes for a row whose symbols are all zero: each tile is its interpolated low-res block
 * (downsampled.cpp:116-169), clamped to 0 .. 255, through the colour inverse (ycbcr.cpp:54-82) where
 * FRMT says YCbCr and C >= 3, clipped at the right and bottom edges as the full decode clips.  k = 0 is
 * a useful result: the low-res plane as a smooth full-size picture.
 * Bytes loaded.  Nothing at or beyond avail rounded up to 4: the bit readers' look-ahead and the
 * 384-byte staging of the FRES tree are bounded by avail as they are bounded by the stream's size in
 * the full decode.
 *
 * Not in this change: a host batch entry; scaled, tensor and pitched forms; himg::Decoder; the
 * multi-GPU handle.
 */
typedef struct himg_hip_prefix_plan {
  int width, height, num_channels;   /* the frame's geometry (FRMT); 0 where FRMT has not arrived */
  int rows;                          /* block rows, ceil(height / 8) */
  int rows_complete;                 /* k */
  size_t packed_size;                /* T (0 where the RIFF header has not arrived) */
  size_t head_bytes;                 /* where the first row header starts */
  size_t used_bytes;                 /* the end of row k-1's payload; head_bytes for k = 0 */
  size_t next_bytes;                 /* the least avail at which a later call could report more rows */
} himg_hip_prefix_plan;
/* Host only, no GPU; reads nothing at or beyond avail.  next_bytes: when the next row's header is wholly
 * present, the end of that row's payload; when the header is cut, the end of the header as far as that
 * is known -- its 2 bytes, or 4 when its first two bytes are present and carry the continuation flag;
 * T when k == rows.  HIMG_ERR_CAPACITY when avail ends before head_bytes (head_bytes set when it is
 * known, else 0, as in himg_hip_preview_peek; the geometry and T are set as far as they have arrived);
 * the other codes are himg_hip_region_peek's.  Like that call it looks at the chunk headers, the length
 * of the FRES tree and the row headers, not into the chunks' bodies. */
int himg_hip_prefix_peek(const uint8_t *packed, size_t avail, int fix_t2, himg_hip_prefix_plan *plan);
/* One prefix in host memory into caller-owned host memory.  The capacity protocol of
 * himg_hip_decode_to: a NULL or too-small dst gives HIMG_ERR_CAPACITY with the geometry and
 * *rows_complete = k set, and himg_hip_fetch_last copies the resident result.  A prefix that ends
 * before head_bytes gives HIMG_ERR_CAPACITY with *rows_complete = -1 (also set on every other
 * failure).  Only avail bytes are read and uploaded. */
int himg_hip_decode_prefix_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t avail, uint8_t *dst,
                              size_t dst_cap, int *width, int *height, int *channels, int *rows_complete);
/* A batch of prefixes in HBM: the contract of himg_hip_decode_device, with h_avail -- a HOST array of
 * the bytes present in each frame -- where h_sizes stands: in_stride is a multiple of 4 and at least
 * every avail rounded up to 4, bytes in [avail_f, in_stride) may hold anything, and the values ride to
 * the device as h_origins do (no host synchronisation: k_f is found on the device).  d_rows[f]
 * receives k_f, -1 on any failure.  A frame below its head_bytes gets d_status[f] =
 * HIMG_ERR_CAPACITY's status and its picture is not written; the other frames are unaffected. */
int himg_hip_decode_prefix_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                  const uint32_t *h_avail, int batch, int width, int height,
                                  int num_channels, void *d_out, int32_t *d_rows, int32_t *d_status,
                                  void *stream);

/* ---- continue a prefix decode: only the block rows that have become whole since the last call ---- */
/*
 * The prefix decode is stateless: every call decodes every complete row again.  A caller who keeps the
 * picture while a stream arrives keeps one himg_hip_prefix_state per picture beside it and calls these
 * entry points instead.
 *
 * The defining property.  For any chain of calls at a_0 <= a_1 <= ... <= a_n on one picture and one state,
 * over a stream whose bytes below each a_i do not change, the picture, d_rows and d_status after the last
 * call are byte for byte those of ONE himg_hip_decode_prefix_device call at a_n (a_n == T: those of
 * himg_hip_decode_device).
 *
 * Per frame, with state s and a bytes present:
 *   - s.started == 0 (a zeroed state is a fresh one): the call IS himg_hip_decode_prefix_device for that
 *     frame -- the same verdict, d_rows and bytes, the whole picture written.  Without a verdict the state
 *     becomes {1, k, the walk's position, a}.  Below head_bytes: HIMG_ERR_CAPACITY's status, the picture
 *     is not written, the state stays zero.
 *   - s.started != 0: the head -- RIFF .. the FRES tree and the whole LRES chain -- runs again with the
 *     prefix decode's verdicts (the context keeps nothing between calls).  The header walk resumes at
 *     s.walk_pos with row s.rows_done and finds k_new >= s.rows_done by the prefix decode's rules.  Only
 *     block rows [s.rows_done, k_new) are entropy-decoded, with the same checks.  WRITTEN: pixel rows
 *     8 s.rows_done .. min(8 k_new, H) - 1 of the frame's picture and NO OTHER BYTE of d_out: no fill, no
 *     row below s.rows_done.  Rows from k_new on keep what the picture held -- the first call's fill.
 *     d_rows[f] = k_new, d_status[f] = 0, the state advances.  No new bytes, or new bytes that complete no
 *     row: nothing of the picture is written.
 *   - A verdict in the new bytes (a header the walk rejects, fewer blocks than rows at the chunk's end, a
 *     new row that fails its checks): the status word himg_hip_decode_prefix_device gives at a,
 *     d_rows[f] = -1, the state is LEFT AS IT WAS (the call repeats with the same verdict).  Pixel rows
 *     from 8 s.rows_done on are unspecified; those above are untouched.
 *   - A state that cannot be right: HIMG_ERR_ARG's status word (1), nothing written, the state left as it
 *     was.  The rules: a < s.avail_seen (judged first, before the head); then, where the head has passed,
 *     rows_done outside [0, rows], walk_pos outside [head_bytes, the end of the FRES chunk], walk_pos > a.
 *     The state is untrusted memory: every field is judged before anything is loaded through it, and the
 *     prefix decode's bound on the bytes loaded holds.  (A state that passes these rules but belongs to
 *     another stream gives that stream's verdicts or pixels, never a load or store out of bounds.)
 *   - walk_pos is himg_hip_prefix_plan::used_bytes of the call that wrote the state.  Where a chunk holds
 *     blocks behind its last block row, their headers are walked again by every call.
 * One launch takes fresh, resumed, idle and below-head frames together.
 *
 * Where it loses: a single call from a fresh state is the prefix decode plus two small kernels, and the
 * head (the parse and the LRES chain) is paid at every step.
 *
 * Not in this change: the command-line tools and himg::Decoder; a host batch form; scaled, tensor, pitched
 * and concealing forms; the multi-GPU handle; keeping the head's products between calls; a cap on the rows
 * decoded per call.
 */
typedef struct himg_hip_prefix_state {   /* 16 bytes; an array of them is 16-byte aligned */
  uint32_t started;      /* 0: nothing decoded yet -- a zeroed state is a fresh one */
  int32_t  rows_done;    /* k: block rows [0, k) of the caller's picture are the full decode's */
  uint32_t walk_pos;     /* where the header walk stands: the first row header not yet passed (the end of
                            the FRES chunk once it has been reached); equals used_bytes while k < rows */
  uint32_t avail_seen;   /* the avail of the last call that advanced this state */
} himg_hip_prefix_state;
/* himg_hip_prefix_peek's result, reached by resuming the walk at *state (host only, no GPU; the chunk
 * headers are checked as there; nothing at or beyond avail is read).  Its codes, plus HIMG_ERR_ARG for a
 * state that cannot be right (the plan is zeroed then).  A fresh state: himg_hip_prefix_peek. */
int himg_hip_prefix_peek_from(const uint8_t *packed, size_t avail, int fix_t2,
                              const himg_hip_prefix_state *state, himg_hip_prefix_plan *plan);
/* A batch in HBM: the layout, in_stride, h_avail, asynchrony and HIMG_OPT_FIX_T2 of
 * himg_hip_decode_prefix_device.  d_state: `batch` states in DEVICE memory, 16-byte aligned, read and
 * updated on the device -- no host round trip learns k, and two calls queued on one stream are ordered by
 * the stream alone: the second consumes what the first wrote.  Bad arguments (a NULL or misaligned d_state,
 * or what himg_hip_decode_prefix_device refuses): HIMG_ERR_ARG, nothing launched. */
int himg_hip_decode_prefix_more_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                       const uint32_t *h_avail, int batch, int width, int height,
                                       int num_channels, himg_hip_prefix_state *d_state, void *d_out,
                                       int32_t *d_rows, int32_t *d_status, void *stream);
/* One prefix in host memory; dst is the caller's full H x W x C picture, *state its state in host memory.
 * A fresh state behaves as himg_hip_decode_prefix_to.  Otherwise only [0, head_bytes) and
 * [state->walk_pos, avail) are uploaded, each at its offset, and only the pixel rows of block rows
 * [k_prev, k_new) are copied back, into their place in dst.  A NULL or too-small dst: HIMG_ERR_CAPACITY
 * with the geometry set, nothing decoded, the state unchanged.  *rows_complete = -1 and the state unchanged
 * on every failure.  Nothing is kept resident: this entry point has NO himg_hip_fetch_last protocol. */
int himg_hip_decode_prefix_more_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t avail,
                                   himg_hip_prefix_state *state, uint8_t *dst, size_t dst_cap,
                                   int *width, int *height, int *channels, int *rows_complete);

/* ---- decode a damaged stream: rejected block rows concealed from the low-res plane ---- */
/*
 * himg_hip_decode rejects a whole picture for one bad block row.  The concealing decode does not: a frame
 * whose HEAD is sound always yields a picture.  Rows the decoder accepts are byte for byte the full
 * decode's; rows it rejects or cannot delimit are written from the low-res plane; the caller learns which
 * rows those were.  Nothing new is defined: a row's verdict is the reference's (huffman_dec.cpp:232-248,
 * :361-417), the fill is the prefix decode's.
 *
 * Head.  RIFF, FRMT, LMAP, LRES (chunk, tree and payload: the whole low-res chain), QCFG, FMAP, the FRES
 *   chunk header, the T2 check (under the same HIMG_OPT_FIX_T2) and the FRES tree run exactly as in the
 *   full decode.  A frame that fails there gets the full decode's d_status[f] (and its
 *   himg_hip_last_error wording in _to) and d_concealed[f] = -1; its row map is not written and its
 *   picture is unspecified, as in himg_hip_decode_device.  Other frames are unaffected.
 * Walk.  The row headers are walked by the decoder's rules from the first one.  k_f is the number of rows
 *   whose header and payload the walk passes before its first failure, at most `rows`.  A failure behind
 *   the last block row (surplus blocks, a header crossing the chunk's end there) conceals nothing.  A frame
 *   of one block row under HIMG_OPT_FIX_T2 has no header: k_f = 1.
 * Rows.  Each row r < k_f is judged on its own with the full decode's checks: the record's total against
 *   the row block, the end-of-block checks, AtTheEnd, an empty payload.  An accepted row's 8 pixel rows
 *   are the full decode's, byte for byte.  A rejected row, and every row r >= k_f, is written as a row of
 *   zero symbols -- exactly the prefix decode's pixels for a row that has not arrived -- and its row-map
 *   byte is 1, otherwise 0.  A row has ONE verdict across the whole width.
 * Results.  d_status[f] = 0; d_concealed[f] = the number of 1s in the frame's row map.
 * A stream himg_hip_decode accepts: the same bytes as himg_hip_decode_device, d_concealed[f] = 0, an
 *   all-zero row map.  Such frames are decoded by the full decode's own kernels; the repair pass behind
 *   them costs a clean batch only its (empty) launches.
 *
 * Two caveats.
 *   - The format has no checksums.  A damaged row the decoder ACCEPTS is decoded as it stands, as the full
 *     decode does today, and a damaged size header that still passes the walk shifts every later row.
 *   - d_concealed[f] == 0 does not prove that the full decode accepts the stream: the surplus-block case
 *     above.
 *
 * Not in this change: a host batch entry; scaled, region, tensor, pitched and pyramid forms; concealment
 * combined with a prefix (avail < T); himg::Decoder; the multi-GPU handle and the row-sharded decode; any
 * smarter concealment than the low-res fill.
 */
/* A batch in HBM: the contract of himg_hip_decode_device for the layout and in_stride, the sizes (they
 * ride to the device without a host wait; the repair pass runs behind the full decode on the same stream),
 * HIMG_OPT_FIX_T2, and the loads: nothing at or beyond h_sizes[f] rounded up to 4.  d_concealed: batch
 * int32; d_rowmap: [batch][rows] bytes, rows = ceil(height / 8), may be NULL.  Bad arguments:
 * HIMG_ERR_ARG, nothing launched. */
int himg_hip_decode_conceal_device(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                                   const uint32_t *h_sizes, int batch, int width, int height,
                                   int num_channels, void *d_out, int32_t *d_concealed, uint8_t *d_rowmap,
                                   int32_t *d_status, void *stream);
/* One host stream into caller-owned host memory.  The capacity protocol of himg_hip_decode_to, with
 * himg_hip_fetch_last: a NULL or too-small dst gives HIMG_ERR_CAPACITY with the geometry, *concealed and
 * the row map set.  The whole stream is uploaded and walked on the device (the host index cannot be built
 * over a bad header).  rowmap (rows bytes) may be NULL; a non-NULL rowmap with rowmap_cap below rows is
 * HIMG_ERR_CAPACITY and nothing is decoded.  *concealed = -1 on every failure. */
int himg_hip_decode_conceal_to(himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, uint8_t *dst,
                               size_t dst_cap, int *width, int *height, int *channels, uint8_t *rowmap,
                               size_t rowmap_cap, int *concealed);

/* ---- row-sharded encode of ONE frame over several GPUs -------------------- */
/*
 * FRES block rows are independently coded units behind size headers
 * (reference huffman_enc.cpp:342-358), so one large frame shards by block rows:
 * rank r owns rows [row0, row1) (multiples of 16 = one low-res macro-block row,
 * except the last).  One context per rank; the host runs the collectives
 * (himg_amd/sharded.py: RCCL via torch.distributed) between the phases:
 *
 *   shard_stats     local rows: colour lift, low-res rows, tiles -> symbols, token
 *                   histogram.  Reads pixel rows [8*row0-11, 8*row1+5) of the
 *                   frame only (d_frame_base may be a virtual base pointer).
 *                   Out: local FRES histogram (261 x u32), low-res rows
 *                   [C][row1-row0][cols].
 *     -> all-reduce(sum) of the histograms; gather of the low-res rows to rank 0
 *   shard_row_bits  Huffman tree from the GLOBAL histogram (identical on every
 *                   rank, reference tie-breaking), payload bits of the local rows.
 *     -> all-gather of the row bit counts
 *   shard_emit      lay out ALL rows relative to the first row header (same on
 *                   every rank), pack the local rows into d_rel (capacity rel_cap >=
 *                   FRES symbols + 4*rows, 16-byte aligned) at those offsets; the
 *                   local byte range follows from the row bit counts
 *                   (himg_amd.sharded.fres_layout).
 *     -> gather of the byte ranges to rank 0
 *   shard_assemble  rank 0: LRES stream from the gathered low-res plane, container,
 *                   FRES tree, the gathered rows, stale pad bits (trap T1).
 * The result is byte-identical to himg_hip_encode of the whole frame.
 */
int himg_hip_shard_stats(himg_hip_ctx *ctx, const void *d_frame_base, int width, int height,
                         int pixel_stride, int num_channels, int quality, int use_ycbcr,
                         int row0, int row1, uint32_t *d_fres_hist, uint8_t *d_low_rows,
                         void *stream);
int himg_hip_shard_row_bits(himg_hip_ctx *ctx, const uint32_t *d_fres_hist_global,
                            uint32_t *d_row_bits, void *stream);
int himg_hip_shard_emit(himg_hip_ctx *ctx, const uint32_t *d_all_row_bits, void *d_rel,
                        size_t rel_cap, uint32_t *d_rel_size, void *stream);
int himg_hip_shard_assemble(himg_hip_ctx *ctx, const uint8_t *d_low_full,
                            const uint32_t *d_all_row_bits, const void *d_rel, size_t rel_bytes,
                            void *d_out, size_t out_cap, uint32_t *d_size, int32_t *d_status,
                            void *stream);
/* The assembling rank in its final-placement form (instead of shard_emit + shard_assemble
 * there): once the row bit counts are known, shard_head builds everything that does not come
 * from another rank straight in the stream buffer d_out -- container, LRES stream from the
 * gathered low-res plane, FRES tree, every row's size header, the payloads of the rank's own
 * rows -- while the peers still pack and send; d_head receives [0] the byte offset of the
 * first row header in d_out and [1] the stream's size, so that the peers' byte ranges
 * (relative to the first row header, himg_amd.sharded.fres_layout) are received in place at
 * d_out + d_head[0] + start.  shard_finish, once every range has arrived: the stale pad bits
 * (trap T1).  d_out: out_cap >= himg_hip_max_packed_size, a multiple of 256, 16-byte aligned. */
int himg_hip_shard_head(himg_hip_ctx *ctx, const uint8_t *d_low_full, const uint32_t *d_all_row_bits,
                        void *d_out, size_t out_cap, uint32_t *d_size, uint32_t *d_head,
                        int32_t *d_status, void *stream);
int himg_hip_shard_finish(himg_hip_ctx *ctx, void *d_out, size_t out_cap, const uint32_t *d_size,
                          void *stream);

/* ---- row-sharded decode of ONE frame over several GPUs -------------------- */
/*
 * Block rows are independently coded (reference decoder.cpp:298-309 hands them
 * to worker threads), so one large frame decodes by block rows too.  Every rank
 * holds the packed stream, parses the container, walks the row headers and
 * decodes the small LRES stream (1/64 of the data); it then decodes only block
 * rows [row0, row1) into d_out_rows = pixel rows [8*row0, min(8*row1, height)),
 * tightly packed.  There is no data-path collective: the verdict is the OR of the
 * ranks' d_status (a stream the reference rejects is rejected by the rank that
 * meets the failing check; container-level failures are seen by every rank).
 * packed_size bytes at d_packed, readable up to the next multiple of 4.
 */
int himg_hip_decode_rows_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                int width, int height, int num_channels, int row0, int row1,
                                void *d_out_rows, int32_t *d_status, void *stream);

/* The same with the stream SCATTERED instead of replicated ("rank 0 parses
 * headers/row index, broadcasts tree + low-res plane ..., scatters row payload slices"):
 *   himg_hip_decode_index_device   on the rank that holds the stream: container parse and
 *       the serial walk over the row size headers (huffman_dec.cpp:232-248), nothing
 *       else.  d_row_index receives [rows] payload byte offsets, then [rows] payload
 *       lengths; *d_rows_first the offset of the first row header.  Bytes
 *       [0, rows_first) -- container chunks, LRES stream, FRES tree -- go to every rank,
 *       bytes [offset[row0] - 4, offset[row1-1] + length[row1-1]) only to the rank that
 *       decodes rows [row0, row1).
 *   himg_hip_index_host            the same index for a stream in host memory (no GPU).
 *   himg_hip_decode_rows_indexed_device   decode rows [row0, row1) from a buffer that holds
 *       those two byte ranges at their offsets in the stream (packed_size is still the
 *       size of the whole stream; nothing else of it is read), with the row index
 *       supplied: no rank repeats the header walk. */
int himg_hip_decode_index_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                 int width, int height, int num_channels, uint32_t *d_row_index,
                                 uint32_t *d_rows_first, int32_t *d_status, void *stream);
int himg_hip_index_host(const uint8_t *packed, size_t packed_size, int fix_t2, int *width, int *height,
                        int *num_channels, uint32_t *row_index, size_t index_rows,
                        uint32_t *rows_first);
int himg_hip_decode_rows_indexed_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                        int width, int height, int num_channels, int row0, int row1,
                                        const uint32_t *d_row_index, void *d_out_rows,
                                        int32_t *d_status, void *stream);
/* The same in two launches, for a rank whose rows' bytes arrive later than the head of the
 * stream (pipelined row-sharded decode): decode_head_device needs only the bytes in front of
 * the first row header -- container parse, LRES chain, predictor inverse --, and
 * decode_rows_after_head_device (same context, stream and geometry) the row index and the
 * rows' bytes.  decode_first_device: where the first row header lies, without the header
 * walk (the rank that holds a stream in HBM sends the head on its way before it indexes). */
int himg_hip_decode_head_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                int width, int height, int num_channels, void *stream);
int himg_hip_decode_rows_after_head_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                           int width, int height, int num_channels, int row0, int row1,
                                           const uint32_t *d_row_index, void *d_out_rows,
                                           int32_t *d_status, void *stream);
int himg_hip_decode_first_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                 int width, int height, int num_channels, uint32_t *d_rows_first,
                                 int32_t *d_status, void *stream);
/* The row index by the header walk alone, on the context's side stream behind what `stream`
 * holds at the call: launched in FRONT of decode_head_device it runs beside the head phase.
 * d_row_index / d_rows_first as himg_hip_decode_index_device, d_status: the walk's verdict
 * (the container's is the head phase's); all valid after himg_hip_decode_walk_wait. */
int himg_hip_decode_walk_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                int width, int height, int num_channels, uint32_t *d_row_index,
                                uint32_t *d_rows_first, int32_t *d_status, void *stream);
int himg_hip_decode_walk_wait(himg_hip_ctx *ctx);
/* The same walk in ROW RANGES, for the rank that scatters a stream over several ranks
 * (replaces, on the device, the serial header walk of huffman_dec.cpp:232-248 as the reference's
 * decoder.cpp:292-326 consumes it row by row): n_ranges launches on the context's side stream,
 * range k ending in front of block row range_end[k] (ascending; the last one >= rows walks to the
 * end).  Behind every range its rows' offsets / lengths are copied to d_row_index ([rows] offsets,
 * then [rows] lengths) and the walk's verdict so far to d_range_status[k]: what a range's owner
 * needs is complete -- and can be sent on its way -- when himg_hip_decode_walk_wait_range(k)
 * returns, while the walk goes on through the ranges behind it.  At most HIMG_MAX_WALK_RANGES. */
#define HIMG_MAX_WALK_RANGES 16
int himg_hip_decode_walk_ranges_device(himg_hip_ctx *ctx, const void *d_packed, uint32_t packed_size,
                                       int width, int height, int num_channels, const int *range_end,
                                       int n_ranges, uint32_t *d_row_index, uint32_t *d_rows_first,
                                       int32_t *d_range_status, void *stream);
int himg_hip_decode_walk_wait_range(himg_hip_ctx *ctx, int k);

/* ---- multi-device: several GPUs of one node behind this ABI ------------------- */
/*
 * One handle over n device slots (one engine context, one stream and one host thread
 * per slot; the same device may be named more than once).  What it replaces in the
 * reference is the decoder's worker pool (decoder.cpp:292-326: block rows handed to
 * threads) -- here the workers are GPUs -- and nothing on the encoder side, which is
 * single-threaded (encoder.cpp:258-335).
 *   himg_hip_multi_encode_batch / _decode_batch   independent frames dealt over the slots
 *       (contiguous shares); per-frame semantics of himg_hip_encode_batch / _decode_batch.
 *       No exchange step.
 *   himg_hip_multi_encode   ONE frame, block rows sharded (multiples of 16 rows): the
 *       histograms (261 x u32) and the row bit counts (rows x u32) meet on the host, the
 *       low-res rows go to slot 0 by peer copy, and every slot packs its rows straight
 *       into slot 0's buffer through peer access (xGMI; without peer access: packed
 *       locally, then one peer copy per slot).  Byte-identical to himg_hip_encode.
 *   himg_hip_multi_decode   ONE frame: the host indexes the block rows
 *       (himg_hip_index_host), every slot receives the head of the stream and only its
 *       own rows' bytes, decodes them and copies its pixel rows into the result.
 *       Accepts and rejects exactly like himg_hip_decode.
 * Frames of fewer than 32 block rows and handles with one slot take the single-device
 * path.  *out of the two one-frame calls is malloc'ed (himg_hip_free).
 * himg::Encoder / himg::Decoder use such a handle when HIMG_DEVICES names more than one
 * device ("0-7", "0,2,4", "0,0": slots on one GPU).
 */
typedef struct himg_hip_multi himg_hip_multi;
int himg_hip_create_multi(const int *devices, int n, himg_hip_multi **out);
void himg_hip_destroy_multi(himg_hip_multi *m);
int himg_hip_multi_count(const himg_hip_multi *m);
const char *himg_hip_multi_last_error(const himg_hip_multi *m);
int himg_hip_multi_set_option(himg_hip_multi *m, int option, int value);
int himg_hip_multi_encode_batch(himg_hip_multi *m, const uint8_t *const *frames, int n, int width,
                                int height, int pixel_stride, int num_channels, int quality,
                                int use_ycbcr, uint8_t *const *dst, const size_t *dst_cap,
                                size_t *out_sizes);
int himg_hip_multi_decode_batch(himg_hip_multi *m, const uint8_t *const *packed,
                                const size_t *packed_sizes, int n, uint8_t *const *dst,
                                const size_t *dst_cap, int *widths, int *heights, int *channels);
int himg_hip_multi_encode(himg_hip_multi *m, const uint8_t *data, int width, int height,
                          int pixel_stride, int num_channels, int quality, int use_ycbcr,
                          uint8_t **out, size_t *out_size);
int himg_hip_multi_decode(himg_hip_multi *m, const uint8_t *packed, size_t packed_size, uint8_t **out,
                          int *width, int *height, int *num_channels);

/* ---- introspection for parity tests and bench.py ------------------------ */

/* Intermediate device buffers of the LAST encode/decode on this context
 * (frame index f of the batch), copied to host.  Synchronises the stream. */
enum {
  HIMG_DBG_AVG = 0,        /* u8  [C][rows][cols] box averages                 */
  HIMG_DBG_LOWRES = 1,     /* u8  [C][rows][cols] low-res plane (m_data)       */
  HIMG_DBG_LRES_SYM = 2,   /* u8  [C][chan_size] LRES payload before entropy   */
  HIMG_DBG_FRES_SYM = 3,   /* u8  [rows][C][64][cols] FRES payload             */
  HIMG_DBG_LRES_HIST = 4,  /* u32 [261] token histogram                        */
  HIMG_DBG_FRES_HIST = 5,  /* u32 [261]                                        */
  HIMG_DBG_LRES_LEN = 6,   /* u32 [261] code lengths                           */
  HIMG_DBG_FRES_LEN = 7,   /* u32 [261]                                        */
  HIMG_DBG_LRES_CODE = 8,  /* u64 [261] LSB-first codes                        */
  HIMG_DBG_FRES_CODE = 9,  /* u64 [261]                                        */
  HIMG_DBG_FRES_ROW_BYTES = 10, /* u32 [rows] payload bytes per block row      */
  HIMG_DBG_DEC_STATS = 11, /* decoder only: u32 [rows+1][8] entropy-decode counters   */
  HIMG_DBG_PARSE_STATS = 12, /* decoder only: u32 [4] container-parse phase cycles / 16 */
  HIMG_DBG_ROWCOUNT_STATS = 13, /* decoder only: u32 [rows][8] k_row_count phase cycles / 16 */
  HIMG_DBG_LOOP_COUNTS = 14 /* u64 [8][2] trip counts of the marked hot loops since the last read (wavefront
                               iterations, lane iterations), encoder or decoder kernels; only in a library
                               built with -DHIMG_LOOP_COUNTS (tools/dynamic_mix.py), HIMG_ERR_ARG otherwise */
  ,
  HIMG_DBG_FRES_TOK_SYM = 15 /* encoder, after a batch encode that went through the token stream (HIMG_OPT_ROW_TOKENS):
                                u8 [rows][C][64][cols], the slots of k_tok expanded into symbols again; status 7 is
                                raised when a row's slots do not cover it exactly */
  ,
  HIMG_DBG_TOK_CNT = 16 /* encoder, after such an encode: u32 [rows][segments] the slots k_tok wrote per token
                           segment of every block row (before the padding of the tail; himg_hip_tok_layout) */
  ,
  HIMG_DBG_LANE_START = 17, /* decoder, after a full decode whose rows went through a count kernel: u32 [rows][1024]
                             where the chain of every lane of a block row starts (bits from the row's payload) */
  HIMG_DBG_LANE_OFF = 18   /* decoder, likewise: u32 [rows][1024 + 72] symbols in front of every lane, then the row's
                             header words (total, end of the chain, valid flag, rounds, records per lane, ...) */
};
int himg_hip_debug_read(himg_hip_ctx *ctx, int what, int frame, void *host_dst,
                        size_t dst_bytes, size_t *bytes_written);

/* The front of himg_hip_decode_device and no more (its argument contract, without d_out): container
 * parse, row-header walk, and the row records of every block row by the wavefront-per-row count kernel
 * in the form HIMG_OPT_COUNT_STRETCH selects, whatever the batch size.  No row kernel runs, no pixel is
 * written; d_status gets the verdict so far.  The records are then read with HIMG_DBG_LANE_START /
 * HIMG_DBG_LANE_OFF: the tests compare the forms of the count kernel word for word this way before a
 * row kernel consumes what a new form writes. */
int himg_hip_debug_row_records(himg_hip_ctx *ctx, const void *d_packed, size_t in_stride,
                               const uint32_t *h_sizes, int batch, int width, int height,
                               int num_channels, int32_t *d_status, void *stream);

/* The encoder's tree kernel (k_tree) alone, on histograms of the caller's: n token histograms of 261
 * counts each (host memory, none of them empty, every total at most 2^31 - 1 like the reference's
 * int counts; 1 <= n <= 16384).  Histogram i is put into BOTH stream slots (0 = LRES, 1 = FRES) of frame
 * i of a scratch workspace of the call's own -- the last encode's buffers are not touched -- and
 * the unchanged kernel runs over them.  All outputs are host arrays: codes [n][2][261] (LSB first),
 * lens [n][2][261], trees [n][2][384] (the serialised tree, zero behind its tree_bytes [n][2] bytes)
 * and status [n] (0, or 3 where a code is longer than 32 bits: what an encode would answer with
 * HIMG_ERR_UNSUPPORTED).  For the tests that hold the kernel against the reference's tree on
 * histograms no picture produces.  Synchronises the device. */
int himg_hip_debug_trees(himg_hip_ctx *ctx, const uint32_t *hist, int n, uint64_t *codes,
                         uint32_t *lens, uint8_t *trees, uint32_t *tree_bytes, int32_t *status);

/* Per-stage device timing with hipEvents recorded on the caller's stream.
 * enable != 0 brackets every kernel of the following calls; stage_ms returns
 * the accumulated milliseconds and launch counts since the last reset. */
#define HIMG_MAX_STAGES 32
int himg_hip_profile_enable(himg_hip_ctx *ctx, int enable);
int himg_hip_profile_reset(himg_hip_ctx *ctx);
int himg_hip_profile_read(himg_hip_ctx *ctx, int *n_stages,
                          const char *names[HIMG_MAX_STAGES],
                          double ms[HIMG_MAX_STAGES], int launches[HIMG_MAX_STAGES]);

/* ---- host utilities (no GPU needed) -------------------------------------- */

/* The token-stream layout of the encoder's FRES rows for a geometry (k_tok -> k_emit_tok):
 * out[0] symbols per segment, out[1] segments per block row, out[2] 16-bit slots a segment owns
 * (its capacity: no content needs more -- the bound of himg_dev.h), out[3] the slots half an
 * iteration of k_tok can stage at most, out[4] the slots its stage holds, out[5] whether an
 * encode of `batch` frames with HIMG_OPT_ROW_TOKENS = row_tokens (-1, 0, 1, 2) takes the token
 * stream: never when out[3] > out[4].  Returns HIMG_ERR_ARG for a geometry the encoder refuses. */
int himg_hip_tok_layout(int width, int height, int pixel_stride, int num_channels, int row_tokens, int batch,
                        int out[6]);

/* Synthetic RGBA generators of SURVEY.md Appendix C.1. */
enum { HIMG_SYNTH_GRAD = 0, HIMG_SYNTH_GRADN = 1, HIMG_SYNTH_RAND = 2, HIMG_SYNTH_RANDTILE = 3 };
int himg_synth_fill(int kind, uint64_t seed, int width, int height, uint8_t *rgba);
uint64_t himg_fnv1a64(const uint8_t *data, size_t n);

/* Host-side format tables (quantize.cpp:72-125, mapper.cpp:75-223); exposed
 * so the parity tests can compare them with the oracle without a GPU. */
void himg_tables_shift(int quality, int chroma, uint8_t out[64]);
void himg_tables_lowres_map(int quality, int16_t out[128]);
void himg_tables_fullres_map(int16_t out[128]);
uint8_t himg_tables_map_to_8bit(const int16_t table[128], int x);

#ifdef __cplusplus
}
#endif
#endif /* HIMG_HIP_H_ */
