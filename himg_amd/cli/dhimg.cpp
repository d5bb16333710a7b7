// dhimg -- decompress a .himg file on the MI355X engine.
//
// Command line, messages and exit codes follow the reference tool
// (src/dhimg.cpp:17-72): "dhimg image outfile"; exit 0 on bad arguments, -1 when
// the input cannot be read, decoded or the output cannot be written.  The picture
// is written as binary PGM / PPM / PAM by channel count (the reference writes PNG
// through FreeImage, which this image does not have).
// One addition: an optional leading "-s2" / "-s4" writes the picture at 1/2 / 1/4 scale
// (himg_hip_decode_scaled_to: the decode the format defines at that scale).
// Another: an optional "-r x,y,w,h" behind it writes only that rectangle -- of the scaled picture
// with a scale (himg_hip_decode_scaled_region_to), of the full-resolution picture on its own
// (himg_hip_decode_region_to).  The rectangle is in the coordinates of the picture as the decoder
// returns it (row 0 = the first decoded row); the window then goes through the same row flip
// and channel swap as a whole picture.  A malformed rectangle is a bad argument (usage, exit 0).
// A third: "-t image outfile" decodes a TRUNCATED file, its size being the bytes that are present
// (himg_hip_decode_prefix_to): the block rows that are whole as the full decode writes them, the rest from
// the low-res plane, and a line "block rows K of N".  Not combined with a scale or a rectangle.
// A fourth: "-m image out.ext" writes the picture pyramid from one decode (himg_hip_decode_pyramid_to):
// the full picture to out.ext and the 1/2-, 1/4- and 1/8-scale pictures to out.L1.ext, out.L2.ext and
// out.L3.ext.  On its own only: with a scale, a rectangle or -t it is a bad argument (usage, exit 0),
// decided before the file is read or the device is opened.
// A fifth: "-c image outfile" decodes a file that may be DAMAGED (himg_hip_decode_conceal_to): the block rows
// the decoder accepts as the full decode writes them, the rows it rejects or cannot delimit from the
// low-res plane, and on stderr a line "concealed N of R block rows" followed, when N > 0, by a line with
// the rows' indices.  Exit status 0 whenever the stream's head is sound.  On its own only, like -m.
// A sixth: "-g image out.pgm" writes plane 0 of the stream as a PGM (himg_hip_decode_planes_to, mask 1): the
// codec's own luma for a colour-space-1 stream of three or four channels, else the first channel.  Only
// that plane is transformed and stored.  The rows go through the same flip as a whole picture.  On its own
// only, like -m.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "decoder.h"
#include "himg_hip.h"
#include "pnm_io.h"

namespace {

int fail(const char *what, const char *path) {
  if (path) printf("%s %s\n", what, path);
  else printf("%s\n", what);
  return -1;
}

// out.ext -> out.L<k>.ext (the extension: behind the last dot of the file's name, if it has one).
std::string level_path(const char *path, int k) {
  std::string p(path);
  const size_t slash = p.find_last_of('/'), dot = p.find_last_of('.');
  const std::string tag = ".L" + std::to_string(k);
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash) || dot == 0) return p + tag;
  return p.substr(0, dot) + tag + p.substr(dot);
}

}  // namespace

int main(int argc, const char **argv) {
  if (argc < 3) {
    printf("Usage: %s image outfile\n", argv[0]);
    return 0;
  }
  // The pyramid: "-m image outfile" and nothing else.
  bool mip = false;
  if (argc >= 4)
    for (int i = 1; i < argc - 2; ++i) mip = mip || std::strcmp(argv[i], "-m") == 0;
  if (mip && !(argc == 4 && std::strcmp(argv[1], "-m") == 0)) {
    printf("Usage: %s image outfile\n", argv[0]);
    return 0;
  }
  // The concealing decode: "-c image outfile" and nothing else.
  bool conceal = false;
  if (argc >= 4)
    for (int i = 1; i < argc - 2; ++i) conceal = conceal || std::strcmp(argv[i], "-c") == 0;
  if (conceal && !(argc == 4 && std::strcmp(argv[1], "-c") == 0)) {
    printf("Usage: %s image outfile\n", argv[0]);
    return 0;
  }
  // Plane 0: "-g image outfile" and nothing else.
  bool grey = false;
  if (argc >= 4)
    for (int i = 1; i < argc - 2; ++i) grey = grey || std::strcmp(argv[i], "-g") == 0;
  if (grey && !(argc == 4 && std::strcmp(argv[1], "-g") == 0)) {
    printf("Usage: %s image outfile\n", argv[0]);
    return 0;
  }
  int scale_log2 = 0;
  if (argc >= 4 && std::strcmp(argv[1], "-s2") == 0) scale_log2 = 1;
  else if (argc >= 4 && std::strcmp(argv[1], "-s4") == 0) scale_log2 = 2;
  const bool prefix = !scale_log2 && argc >= 4 && std::strcmp(argv[1], "-t") == 0;
  int arg = scale_log2 || prefix || mip || conceal || grey ? 2 : 1;
  bool region = false;
  int rx = 0, ry = 0, rw = 0, rh = 0;
  if (!prefix && argc >= arg + 4 && std::strcmp(argv[arg], "-r") == 0) {
    char tail = 0;
    if (std::sscanf(argv[arg + 1], "%d,%d,%d,%d%c", &rx, &ry, &rw, &rh, &tail) != 4) {
      printf("Usage: %s image outfile\n", argv[0]);
      return 0;
    }
    region = true;
    arg += 2;
  }
  const char *in_path = argv[arg], *out_path = argv[arg + 1];

  std::vector<uint8_t> stream;
  if (!pnm::slurp(in_path, &stream)) return fail("Unable to read file", in_path);
  printf("File size: %zu\n", stream.size());
  fflush(stdout);   // the library reports through std::cout

  if (mip) {
    int w = 0, h = 0, c = 0;
    if (himg_hip_peek(stream.data(), stream.size(), &w, &h, &c) != HIMG_OK) return fail("Unable to decode image.", nullptr);
    std::vector<uint8_t> pixels[4];
    uint8_t *dst[4];
    size_t cap[4];
    int lw[4], lh[4];
    for (int k = 0; k < 4; ++k) {
      (void)himg_hip_pyramid_size(w, h, k, &lw[k], &lh[k]);
      pixels[k].resize(static_cast<size_t>(lw[k]) * lh[k] * c);
      dst[k] = pixels[k].data();
      cap[k] = pixels[k].size();
    }
    himg_hip_ctx *ctx = nullptr;
    if (himg_hip_create(0, &ctx) != HIMG_OK) return fail("Error: no usable MI355X device (the HIMG engine has no CPU fallback).", nullptr);
    const int rc = himg_hip_decode_pyramid_to(ctx, stream.data(), stream.size(), dst, cap, &w, &h, &c);
    if (rc != HIMG_OK) {
      const char *msg = himg_hip_last_error(ctx);
      printf("%s%s", msg, (*msg && msg[std::strlen(msg) - 1] == '\n') ? "" : "\n");
      himg_hip_destroy(ctx);
      return fail("Unable to decode image.", nullptr);
    }
    himg_hip_destroy(ctx);
    const bool writable = c == 1 || c == 3 || c == 4;
    for (int k = 0; k < 4; ++k) {
      pnm::Image picture;
      picture.width = lw[k];
      picture.height = lh[k];
      picture.channels = c;
      picture.data.resize(pixels[k].size());
      pnm::flip_and_swap(pixels[k].data(), picture.data.data(), lw[k], lh[k], c);
      const std::string path = k ? level_path(out_path, k) : std::string(out_path);
      if (!writable || !pnm::write(path.c_str(), picture)) return fail("Unable to write file", path.c_str());
    }
    return 0;
  }

  if (conceal) {
    int w = 0, h = 0, c = 0, n = -1;
    if (himg_hip_peek(stream.data(), stream.size(), &w, &h, &c) != HIMG_OK) return fail("Unable to decode image.", nullptr);
    const int rows = (h + 7) / 8;
    std::vector<uint8_t> pixels(static_cast<size_t>(w) * h * c), rowmap(static_cast<size_t>(rows));
    himg_hip_ctx *ctx = nullptr;
    if (himg_hip_create(0, &ctx) != HIMG_OK) return fail("Error: no usable MI355X device (the HIMG engine has no CPU fallback).", nullptr);
    const int rc = himg_hip_decode_conceal_to(ctx, stream.data(), stream.size(), pixels.data(), pixels.size(), &w, &h, &c,
                                              rowmap.data(), rowmap.size(), &n);
    if (rc != HIMG_OK) {
      const char *msg = himg_hip_last_error(ctx);
      printf("%s%s", msg, (*msg && msg[std::strlen(msg) - 1] == '\n') ? "" : "\n");
      himg_hip_destroy(ctx);
      return fail("Unable to decode image.", nullptr);
    }
    himg_hip_destroy(ctx);
    fprintf(stderr, "concealed %d of %d block rows\n", n, rows);
    if (n > 0) {
      bool first = true;
      for (int r = 0; r < rows; ++r)
        if (rowmap[r]) { fprintf(stderr, "%s%d", first ? "" : " ", r); first = false; }
      fprintf(stderr, "\n");
    }
    pnm::Image picture;
    picture.width = w;
    picture.height = h;
    picture.channels = c;
    picture.data.resize(pixels.size());
    pnm::flip_and_swap(pixels.data(), picture.data.data(), w, h, c);
    const bool writable = c == 1 || c == 3 || c == 4;
    if (!writable || !pnm::write(out_path, picture)) return fail("Unable to write file", out_path);
    return 0;
  }

  if (grey) {
    int w = 0, h = 0, c = 0;
    if (himg_hip_peek(stream.data(), stream.size(), &w, &h, &c) != HIMG_OK) return fail("Unable to decode image.", nullptr);
    std::vector<uint8_t> plane(static_cast<size_t>(w) * h);
    himg_hip_ctx *ctx = nullptr;
    if (himg_hip_create(0, &ctx) != HIMG_OK) return fail("Error: no usable MI355X device (the HIMG engine has no CPU fallback).", nullptr);
    const int rc = himg_hip_decode_planes_to(ctx, stream.data(), stream.size(), 1u, plane.data(), plane.size(), &w, &h, &c);
    if (rc != HIMG_OK) {
      const char *msg = himg_hip_last_error(ctx);
      printf("%s%s", msg, (*msg && msg[std::strlen(msg) - 1] == '\n') ? "" : "\n");
      himg_hip_destroy(ctx);
      return fail("Unable to decode image.", nullptr);
    }
    himg_hip_destroy(ctx);
    pnm::Image picture;
    picture.width = w;
    picture.height = h;
    picture.channels = 1;
    picture.data.resize(plane.size());
    pnm::flip_and_swap(plane.data(), picture.data.data(), w, h, 1);
    if (!pnm::write(out_path, picture)) return fail("Unable to write file", out_path);
    return 0;
  }

  if (scale_log2 || region || prefix) {
    himg_hip_ctx *ctx = nullptr;
    if (himg_hip_create(0, &ctx) != HIMG_OK) return fail("Error: no usable MI355X device (the HIMG engine has no CPU fallback).", nullptr);
    pnm::Image picture;
    int w = 0, h = 0, c = 0;
    std::vector<uint8_t> pixels;
    int rc, rows_complete = -1;
    if (prefix) rc = himg_hip_decode_prefix_to(ctx, stream.data(), stream.size(), nullptr, 0, &w, &h, &c, &rows_complete);
    else if (!region) rc = himg_hip_decode_scaled_to(ctx, stream.data(), stream.size(), scale_log2, nullptr, 0, &w, &h, &c);
    else if (scale_log2)
      rc = himg_hip_decode_scaled_region_to(ctx, stream.data(), stream.size(), scale_log2, rx, ry, rw, rh, nullptr, 0, &w, &h, &c);
    else rc = himg_hip_decode_region_to(ctx, stream.data(), stream.size(), rx, ry, rw, rh, nullptr, 0, &w, &h, &c);
    if (rc == HIMG_ERR_CAPACITY && !(prefix && rows_complete < 0)) {   // (a prefix below its first row header: an error)
      size_t n = 0;
      pixels.resize(static_cast<size_t>(w) * h * c);
      rc = himg_hip_fetch_last(ctx, pixels.data(), pixels.size(), &n);
    }
    if (rc != HIMG_OK) {
      const char *msg = himg_hip_last_error(ctx);
      printf("%s%s", msg, (*msg && msg[std::strlen(msg) - 1] == '\n') ? "" : "\n");
      himg_hip_destroy(ctx);
      return fail("Unable to decode image.", nullptr);
    }
    himg_hip_destroy(ctx);
    if (prefix) printf("block rows %d of %d\n", rows_complete, (h + 7) / 8);
    picture.width = w;
    picture.height = h;
    picture.channels = c;
    picture.data.resize(pixels.size());
    pnm::flip_and_swap(pixels.data(), picture.data.data(), w, h, c);
    const bool writable = c == 1 || c == 3 || c == 4;
    if (!writable || !pnm::write(out_path, picture)) return fail("Unable to write file", out_path);
    return 0;
  }

  himg::Decoder decoder;
  if (!decoder.Decode(stream.data(), static_cast<int>(stream.size()))) return fail("Unable to decode image.", nullptr);

  // The codec hands back FreeImage's memory convention (bottom-up, BGR(A)); files
  // are top-down RGB(A).
  pnm::Image picture;
  picture.width = decoder.width();
  picture.height = decoder.height();
  picture.channels = decoder.num_channels();
  picture.data.resize(static_cast<size_t>(decoder.unpacked_size()));
  pnm::flip_and_swap(decoder.unpacked_data(), picture.data.data(), picture.width, picture.height, picture.channels);
  const bool writable = picture.channels == 1 || picture.channels == 3 || picture.channels == 4;
  if (!writable || !pnm::write(out_path, picture)) return fail("Unable to write file", out_path);
  return 0;
}
