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
#include <cstdio>
#include <cstring>
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

}  // namespace

int main(int argc, const char **argv) {
  if (argc < 3) {
    printf("Usage: %s image outfile\n", argv[0]);
    return 0;
  }
  int scale_log2 = 0;
  if (argc >= 4 && std::strcmp(argv[1], "-s2") == 0) scale_log2 = 1;
  else if (argc >= 4 && std::strcmp(argv[1], "-s4") == 0) scale_log2 = 2;
  const bool prefix = !scale_log2 && argc >= 4 && std::strcmp(argv[1], "-t") == 0;
  int arg = scale_log2 || prefix ? 2 : 1;
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
