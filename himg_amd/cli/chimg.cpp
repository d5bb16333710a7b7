// chimg -- compress a picture to .himg on the MI355X engine.
//
// Command line, messages and exit codes follow the reference tool
// (src/chimg.cpp:36-169): "chimg [-q N] [-rgb] image outfile"; exit 0 after the
// usage text, -1 when the input cannot be read or the output cannot be written.
// Input: binary PGM / PPM / PAM (pnm_io.h) instead of the formats FreeImage reads.
// Beyond the reference: "-b <bytes>" encodes to a byte budget through the C ABI
// (himg_hip_encode_budget_to, qualities 0 .. the -q value, 100 without one) and prints
// the quality it chose; "-p <dB>" encodes to a quality floor (himg_hip_encode_target_to with
// himg_hip_psnr_to_sse's target) and prints the chosen quality and the PSNR reached;
// "-r x,y,w,h" (the spelling of dhimg -r) encodes only that rectangle (himg_hip_encode_window_to: only
// its rows are uploaded).  As there, the rectangle is in the coordinates of the picture as the codec
// sees it (row 0 = the first coded row, the picture's bottom scanline): dhimg -r of the whole file
// and dhimg of the -r file show the same pixels.  A malformed rectangle is a bad argument (usage).
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "encoder.h"
#include "himg_hip.h"
#include "pnm_io.h"

namespace {

struct Request {
  int quality = 50;        // the reference's default (src/chimg.cpp:22)
  bool ycbcr = true;
  bool have_quality = false;
  long long budget = -1;   // -b: at most this many bytes (-1: not given)
  double psnr = -1.0;      // -p: at least this many dB (-1: not given)
  bool region = false;     // -r: only this rectangle
  int rx = 0, ry = 0, rw = 0, rh = 0;
  const char *input = nullptr;
  const char *output = nullptr;
};

// Returns false (after the reference's message, if any) when the usage text is due.
bool parse(int argc, const char **argv, Request *rq) {
  int nfiles = 0;
  for (int i = 1; i < argc; ++i) {
    const char *a = argv[i];
    if (a[0] != '-') {
      if (nfiles == 0) rq->input = a;
      else if (nfiles == 1) rq->output = a;
      ++nfiles;
    } else if (!strcmp(a, "-rgb")) {
      rq->ycbcr = false;
    } else if (!strcmp(a, "-q")) {
      if (++i >= argc) return false;
      char *end = nullptr;
      const long v = strtol(argv[i], &end, 10);
      if (end == argv[i] || *end) {
        printf("Invalid integer expression: %s\n", argv[i]);
        return false;
      }
      rq->quality = static_cast<int>(v);
      if (v < 0 || v > 100) {
        printf("Invalid quality level: %d\n", rq->quality);
        return false;
      }
      rq->have_quality = true;
    } else if (!strcmp(a, "-b")) {
      if (++i >= argc) return false;
      char *end = nullptr;
      errno = 0;
      const long long v = strtoll(argv[i], &end, 10);
      if (end == argv[i] || *end) {
        printf("Invalid integer expression: %s\n", argv[i]);
        return false;
      }
      if (v < 0 || errno == ERANGE) {
        printf("Invalid byte budget: %s\n", argv[i]);
        return false;
      }
      rq->budget = v;
    } else if (!strcmp(a, "-p")) {
      if (++i >= argc) return false;
      char *end = nullptr;
      const double v = strtod(argv[i], &end);
      if (end == argv[i] || *end) {
        printf("Invalid number: %s\n", argv[i]);
        return false;
      }
      if (!std::isfinite(v) || v < 0.0) {
        printf("Invalid PSNR: %s\n", argv[i]);
        return false;
      }
      rq->psnr = v;
    } else if (!strcmp(a, "-r")) {
      if (++i >= argc) return false;
      char tail = 0;
      if (sscanf(argv[i], "%d,%d,%d,%d%c", &rq->rx, &rq->ry, &rq->rw, &rq->rh, &tail) != 4) {
        printf("Invalid rectangle: %s\n", argv[i]);
        return false;
      }
      rq->region = true;
    } else {
      printf("Invalid option: %s\n", a);
      return false;
    }
  }
  if (rq->budget >= 0 && rq->psnr >= 0.0) {
    printf("-b and -p exclude each other\n");
    return false;
  }
  if (rq->region && (rq->budget >= 0 || rq->psnr >= 0.0)) {
    printf("-r excludes -b and -p\n");
    return false;
  }
  return nfiles == 2;
}

}  // namespace

int main(int argc, const char **argv) {
  Request rq;
  if (!parse(argc, argv, &rq)) {
    printf("Usage: %s [options] image outfile\n"
           "Options:\n"
           " -q <quality> Set the quality (0-100)\n"
           " -rgb         Use RGB color space (instead of YCbCr)\n"
           " -b <bytes>   Fit the file into a byte budget (-q: the highest quality to try)\n"
           " -p <dB>      Reach at least this PSNR in as few bytes as the search finds (-q: as for -b)\n"
           " -r x,y,w,h   Compress only this rectangle (row 0: the first coded row, as dhimg -r)\n",
           argv[0]);
    return 0;
  }

  pnm::Image picture;
  switch (pnm::read(rq.input, &picture)) {
    case 0: break;
    case 2: fprintf(stderr, "Unknown file format for %s\n", rq.input); return -1;
    default: fprintf(stderr, "Unable to load %s\n", rq.input); return -1;
  }
  // The reference hands the codec FreeImage's memory layout (bottom-up scanlines,
  // BGR(A)); do the same so that both tools make the same stream of one picture.
  std::vector<uint8_t> pixels(picture.data.size());
  pnm::flip_and_swap(picture.data.data(), pixels.data(), picture.width, picture.height, picture.channels);

  const int c = picture.channels;
  if (rq.psnr >= 0.0) {
    himg_hip_ctx *ctx = nullptr;
    const size_t cap = himg_hip_max_packed_size(picture.width, picture.height, c);
    std::vector<uint8_t> packed(cap);
    size_t n = 0;
    int quality = -1;
    uint64_t target = 0, sse = 0;
    int rc = himg_hip_psnr_to_sse(rq.psnr, picture.width, picture.height, c, &target);
    if (rc == HIMG_OK) rc = himg_hip_create(0, &ctx);
    if (rc == HIMG_OK)
      rc = himg_hip_encode_target_to(ctx, pixels.data(), picture.width, picture.height, c, c, 0,
                                     rq.have_quality ? rq.quality : 100, rq.ycbcr ? 1 : 0, target, packed.data(),
                                     packed.size(), &n, &quality, &sse);
    himg_hip_destroy(ctx);
    const double samples = (double)picture.width * picture.height * c;
    const double reached = sse ? 10.0 * log10(255.0 * 255.0 * samples / (double)sse) : INFINITY;
    if (rc == HIMG_ERR_TARGET) {
      fprintf(stderr, "%s does not reach %g dB at quality %d (%.2f dB)\n", rq.input, rq.psnr,
              rq.have_quality ? rq.quality : 100, reached);
      return -1;
    }
    if (rc != HIMG_OK) {
      fprintf(stderr, "Unable to encode %s\n", rq.input);
      return -1;
    }
    printf("Quality: %d\n", quality);
    printf("PSNR: %.2f\n", reached);
    printf("Compressed size: %d\n", static_cast<int>(n));
    FILE *f = fopen(rq.output, "wb");
    const bool ok = f && fwrite(packed.data(), 1, n, f) == n;
    if (f) fclose(f);
    return ok ? 0 : -1;
  }
  if (rq.budget >= 0) {
    himg_hip_ctx *ctx = nullptr;
    const size_t cap = himg_hip_max_packed_size(picture.width, picture.height, c);
    std::vector<uint8_t> packed(cap);
    size_t n = 0;
    int quality = -1;
    int rc = himg_hip_create(0, &ctx);
    if (rc == HIMG_OK)
      rc = himg_hip_encode_budget_to(ctx, pixels.data(), picture.width, picture.height, c, c, 0,
                                     rq.have_quality ? rq.quality : 100, rq.ycbcr ? 1 : 0,
                                     static_cast<size_t>(rq.budget), packed.data(), packed.size(), &n, &quality);
    himg_hip_destroy(ctx);
    if (rc == HIMG_ERR_CAPACITY && quality < 0) {
      fprintf(stderr, "%s does not fit %lld bytes at quality 0\n", rq.input, rq.budget);
      return -1;
    }
    if (rc != HIMG_OK) {
      fprintf(stderr, "Unable to encode %s\n", rq.input);
      return -1;
    }
    printf("Quality: %d\n", quality);
    printf("Compressed size: %d\n", static_cast<int>(n));
    FILE *f = fopen(rq.output, "wb");
    const bool ok = f && fwrite(packed.data(), 1, n, f) == n;
    if (f) fclose(f);
    return ok ? 0 : -1;
  }

  if (rq.region) {
    himg_hip_ctx *ctx = nullptr;
    const himg_hip_src src = {picture.width, picture.height, c, (size_t)picture.width * c, 0};
    std::vector<uint8_t> packed(rq.rw > 0 && rq.rh > 0 ? himg_hip_max_packed_size(rq.rw, rq.rh, c) : 0);
    size_t n = 0;
    int rc = himg_hip_create(0, &ctx);
    if (rc == HIMG_OK)
      rc = himg_hip_encode_window_to(ctx, pixels.data(), &src, c, rq.rx, rq.ry, rq.rw, rq.rh, rq.quality,
                                     rq.ycbcr ? 1 : 0, packed.data(), packed.size(), &n);
    himg_hip_destroy(ctx);
    if (rc == HIMG_ERR_ARG) {
      fprintf(stderr, "The rectangle %d,%d,%d,%d does not lie inside %s\n", rq.rx, rq.ry, rq.rw, rq.rh, rq.input);
      return -1;
    }
    if (rc != HIMG_OK) {
      fprintf(stderr, "Unable to encode %s\n", rq.input);
      return -1;
    }
    printf("Compressed size: %d\n", static_cast<int>(n));
    FILE *f = fopen(rq.output, "wb");
    const bool ok = f && fwrite(packed.data(), 1, n, f) == n;
    if (f) fclose(f);
    return ok ? 0 : -1;
  }

  fflush(stdout);   // the library reports through std::cout
  himg::Encoder encoder;
  if (!encoder.Encode(pixels.data(), picture.width, picture.height, c, c, rq.quality, rq.ycbcr)) {
    fprintf(stderr, "Unable to encode %s\n", rq.input);   // no GPU engine: there is no CPU fallback
    return -1;
  }
  printf("Compressed size: %d\n", encoder.packed_size());

  FILE *f = fopen(rq.output, "wb");
  const size_t n = static_cast<size_t>(encoder.packed_size());
  const bool ok = f && fwrite(encoder.packed_data(), 1, n, f) == n;
  if (f) fclose(f);
  return ok ? 0 : -1;
}
