// The front of k_tile_inv and of its tensor, pitched, pyramid and planes forms (k_tile_inv_t / _p / _m / _c): one
// copy, included behind each kernel's own binding of g, ws and v0 (parameters of k_tile_inv, members of
// the other kernels' argument structs), so that every kernel keeps its code instruction for instruction.
// It leaves the block row v, the frame f and its DecFrame df, the tables in LDS and the lane's
// (tile, half) `it`; the lanes beyond the row's last tile have returned.  Each kernel's stores follow.
  __shared__ int16_t s_unmap[256];   // indexed by the code byte
  __shared__ uint8_t s_shift[2][64];
  __shared__ uint32_t s_shiftp[2 * 32 + 4];   // [chroma][register pair], then the identity-test words
  const int v = blockIdx.y + v0, f = blockIdx.z;
  const DecFrame *df = ws.frames + f;
  __shared__ int s_status;
  if (threadIdx.x == 0) s_status = df->status;
  __syncthreads();
  if (s_status) return;
  {
    const int k = threadIdx.x;
    const int sc = (int8_t)k;
    s_unmap[k] = (int16_t)(sc >= 0 ? df->fmap[sc] : (sc == -128 ? -df->fmap[127] : -df->fmap[-sc]));
    if (k < 128) s_shift[k >> 6][k & 63] = df->shift[k >> 6][k & 63];
    if (k < 64) {
      const int ch = k >> 5, e = k & 31, x = e >> 2, j = e & 3;
      s_shiftp[ch * 32 + e] = (uint32_t)df->shift[ch][(2 * j) * 8 + x] | ((uint32_t)df->shift[ch][(2 * j + 1) * 8 + x] << 16);
    }
    if (FAST && k >= 192) identity_test_words(df, k - 192, s_shiftp + 64);
  }
  __syncthreads();
  const int it = blockIdx.x * 256 + threadIdx.x;   // (tile, half): both lanes of a pair are in or out
  if (pair_tile(it) >= g.cols) return;
