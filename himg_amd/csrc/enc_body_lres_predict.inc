  // FOUR macro blocks per wavefront, 16 lanes each (lane & 15 = row of the block):
  // the delta chain only ever has 16 rows to work on, so one block per wave left
  // three quarters of it idle -- and a 4096x4096 frame is 4096 blocks per channel.
  __shared__ __attribute__((aligned(4))) uint8_t mb[4][16][20];   // (rows dword aligned: the fast path stores them as dwords)
  __shared__ uint8_t recp[4][17][18];   // the reconstructed block with a border row / column in front (see the chain below)
  // The companding tables in LDS: the delta chain below looks them up twice per
  // step, and out of the kernel-argument segment each lookup is a global load on
  // the critical path of 31 dependent steps.
  __shared__ int16_t s_tab[128];
  __shared__ uint8_t s_code[512];
  const int lane = threadIdx.x, b = lane >> 4, dv = lane & 15;
  const int mu = blockIdx.x * 4 + b, mv = blockIdx.y;
  const int f = blockIdx.z / g.C, c = blockIdx.z % g.C;
  if constexpr (QI) {
    // (the frame's entry: a uniform base, the lanes' own elements of it on their way into the LDS)
    const LresTables *__restrict__ q = &qual_entry(lt, f)->lt;
    for (int k = lane; k < 128; k += 64) s_tab[k] = q->tab[k];
    for (int k = lane; k < 512; k += 64) s_code[k] = q->code[k];
  } else {
    for (int k = lane; k < 128; k += 64) s_tab[k] = lt.tab[k];
    for (int k = lane; k < 512; k += 64) s_code[k] = lt.code[k];
  }
  const uint8_t *m = low + (size_t)f * plane_stride + (size_t)c * g.rows * g.cols;
  const bool live = mu < g.mcols;
  const int u0 = mu * 16, v0 = mv * 16;
  const int bw = live ? min(16, g.cols - u0) : 0, bh = min(16, g.rows - v0);

  int err[5] = {0, 0, 0, 0, 0};
  // Four full blocks in rows of sixteen-byte-aligned samples (every block of the BASELINE frames
  // but those at the right / bottom edge of odd sizes): the lane's row is ONE 16-byte load and stays
  // in registers, the row above comes from the lane before by DPP (a block is a DPP row of 16
  // lanes), and the predictors' squared errors are accumulated without a branch or an LDS read.
  const bool fast = __all(live && bw == 16 && bh == 16) && (g.cols & 15) == 0;
  if (fast) {
    const uint4 q = *reinterpret_cast<const uint4 *>(m + (size_t)(v0 + dv) * g.cols + u0);
    const uint32_t R[4] = {q.x, q.y, q.z, q.w};
    uint32_t U[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      U[k] = dpp_row_shr1(R[k]);
      *reinterpret_cast<uint32_t *>(&mb[b][dv][4 * k]) = R[k];
    }
    const bool up_ok1 = dv > 0;
#pragma unroll
    for (int du = 0; du < 16; ++du) {
      const int actual = (int)((R[du >> 2] >> (8 * (du & 3))) & 255u);
      const int up = (int)((U[du >> 2] >> (8 * (du & 3))) & 255u);
      int s1, s2, s3;
      if (du > 0) {
        const int left = (int)((R[(du - 1) >> 2] >> (8 * ((du - 1) & 3))) & 255u);
        const int ul = (int)((U[(du - 1) >> 2] >> (8 * ((du - 1) & 3))) & 255u);
        s3 = left; s2 = up_ok1 ? up : left; s1 = up_ok1 ? ul : left;
      } else {
        s1 = s2 = s3 = up_ok1 ? up : 128;
      }
      const int t = s2 + s3;
      const int pr[5] = {clamp255((3 * t - 2 * s1 + 2) >> 2), s2, s3, (t + 1) >> 1, clamp255(t - s1)};
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        const int dd = actual - pr[p];
        err[p] += dd * dd;
      }
    }
    __syncthreads();
  } else {
#pragma unroll
  for (int du = 0; du < 16; ++du)
    mb[b][dv][du] = (dv < bh && du < bw) ? m[(size_t)(v0 + dv) * g.cols + u0 + du] : 0;
  __syncthreads();

  if (dv < bh) {
    for (int du = 0; du < bw; ++du) {
      int s1, s2, s3;
      if (du > 0 && dv > 0) { s1 = mb[b][dv - 1][du - 1]; s2 = mb[b][dv - 1][du]; s3 = mb[b][dv][du - 1]; }
      else if (du > 0) { s1 = s2 = s3 = mb[b][dv][du - 1]; }
      else if (dv > 0) { s1 = s2 = s3 = mb[b][dv - 1][du]; }
      else { s1 = s2 = s3 = 128; }
      const int actual = mb[b][dv][du];
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        const int d = actual - predict(s1, s2, s3, p);
        err[p] += d * d;
      }
    }
  }
  }
#pragma unroll
  for (int p = 0; p < 5; ++p)
    for (int d = 8; d >= 1; d >>= 1) err[p] += __shfl_xor(err[p], d);   // over the block's 16 lanes
  int best = 0, best_err = err[0];
#pragma unroll
  for (int p = 1; p < 5; ++p)
    if (err[p] < best_err) { best = p; best_err = err[p]; }

  uint8_t *out = lres_sym + (size_t)f * lres_stride + (size_t)c * g.chan_size;
  if (live && dv == 0) out[mv * g.mcols + mu] = (uint8_t)(best - 2);  // downsampled.cpp:33-35
  // The stored byte is read back as (uint8 + 2) in int arithmetic
  // (downsampled.cpp:37-39), so selections 0 and 1 both CODE with predictor 0.
  const int pc = best <= 1 ? 0 : best;

  uint8_t *dst = out + g.mrows * g.mcols + (size_t)v0 * g.cols + (size_t)bh * u0;
  // The delta chain, branch free: the three reconstructed neighbours are read from a copy of the
  // block with a border (index + 1: the reads of row / column -1 land on it, their values are
  // not used), the cases of downsampled.cpp:263-281 are four selects (f = the neighbour that
  // stands for all three at an edge), all five predictors are computed and the block's is
  // selected -- the four blocks of a wavefront code with different predictors, and a switch ran
  // every case taken by any of them.  (~100 -> ~45 instructions per anti-diagonal step.)
  const bool row_live = dv < bh;
  const bool up_ok = dv > 0;
  uint8_t *rrow = &recp[b][dv + 1][1];          // rrow[du] = reconstructed sample (dv, du)
  const uint8_t *urow = &recp[b][dv][1];        // the row above
  uint8_t *rec_row = nullptr;                   // REC: the lane's row of the block in the stored plane
  if constexpr (REC)
    rec_row = rec_plane + (size_t)f * plane_stride + (size_t)c * g.rows * g.cols + (size_t)(v0 + (row_live ? dv : 0)) * g.cols + u0;
  for (int d = 0; d < 31; ++d) {
    const int du = d - dv;
    const bool active = row_live && du >= 0 && du < bw;
    const int duc = active ? du : 0;
    const int left = rrow[duc - 1], up = urow[duc], ul = urow[duc - 1];
    const bool left_ok = duc > 0;
    const int f = up_ok ? up : (left_ok ? left : 128);
    const int s3 = left_ok ? left : f, s2 = f, s1 = (up_ok && left_ok) ? ul : f;
    const int t = s2 + s3;
    const int p0 = clamp255((3 * t - 2 * s1 + 2) >> 2), p3 = (t + 1) >> 1, p4 = clamp255(t - s1);
    const int predicted = pc == 2 ? s3 : pc == 3 ? p3 : pc == 4 ? p4 : p0;   // (pc is 0, 2, 3 or 4: selections 0 and 1 both code with 0)
    const int delta = (int)mb[b][dv][duc] - predicted;
    const uint8_t code = s_code[delta + 255];
    const int sc = (int8_t)code;
    const int mag = s_tab[sc < 0 ? -sc : sc];
    const int un = sc < 0 ? -mag : mag;
    if (active) {
      rrow[du] = (uint8_t)clamp255(predicted + un);
      dst[dv * bw + du] = code;
      if constexpr (REC) rec_row[du] = (uint8_t)clamp255(predicted + un);
    }
    __syncthreads();
  }
