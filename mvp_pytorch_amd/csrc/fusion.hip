// fusion.hip — the concat-and-dropout stages of the BiImageBertForSequenceClassificationPlus head
// (oscar/modeling/modeling_vlbert.py:2040-2043) and the ReLU backward of its f32 GEMMs.
//
//   CAT2   out[r, :] = dropout([a_r, b_r])                       torch.cat([pooled_output, single_hidden], 1)   vl:2043
//   PAIR4  out[r, :] = dropout([a_r, b_r, b_r - a_r, b_r * a_r])  a = global_txt, b = global_img                  vl:2040-2041
//
// B rows of a few thousand f32 columns: bandwidth-trivial, what counts is the launch count (torch: cat, sub, mul,
// dropout and their four backward kernels per stage) and that the masks are the documented ones.  One 256-thread
// workgroup per 1024-column piece of a row; a lane owns 4 adjacent columns of EVERY segment, so a, b (and dout in the
// backward pass) are read once and every segment is written from registers.  Fast path: 16-byte loads / stores and
// one hash per element pair, the pairs' chains interleaved (pair_hashes); scalar path (P % 4 != 0, odd strides or
// bases): one element at a time — with odd P an element pair straddles two segments, which the per-element form
// (mvptr_rand16 on the flat index r * W + c) handles by construction.
#include "common.h"

namespace {

struct FuseArgs {
  const float* a;
  const float* b;
  const float* dout;   // backward only
  float* out;          // forward only
  float* da;           // backward only
  float* db;
  int64_t lda, ldb, ldo, ldd, ldda, lddb;
  int rows, P, nseg;   // nseg = 2 (CAT2) or 4 (PAIR4)
  DropDev drop;
};

// f = keep * scale as produced by fuse_factors: a dropped element is 0 whatever v holds (a select like drop_apply, not v * 0)
__device__ __forceinline__ float fuse_keep(float v, float f) { return f != 0.f ? v * f : 0.f; }

// keep * scale of the 4 adjacent columns c0..c0+3 of each segment (fast path: r * W + s * P + c0 is a multiple of 4)
template <int NSEG>
__device__ __forceinline__ void fuse_factors(const DropDev& d, int64_t W, int P, int r, int c0, float (&f)[NSEG][4]) {
  if (d.thresh16 == 0) {
#pragma unroll
    for (int s = 0; s < NSEG; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) f[s][j] = 1.f;
    return;
  }
  uint64_t pair[2 * NSEG];
  uint32_t x[2 * NSEG];
#pragma unroll
  for (int s = 0; s < NSEG; ++s) {
    const uint64_t e = (uint64_t)r * (uint64_t)W + (uint64_t)s * (uint64_t)P + (uint64_t)c0;
    pair[2 * s] = e >> 1;
    pair[2 * s + 1] = (e >> 1) + 1;
  }
  pair_hashes<2 * NSEG, true>(pair, d.seed_lo, d.seed_hi, x);   // the host checked rows * W < 2^33
#pragma unroll
  for (int s = 0; s < NSEG; ++s) {
    f[s][0] = ((x[2 * s] & 0xffffu) >= d.thresh16) ? d.scale : 0.f;
    f[s][1] = ((x[2 * s] >> 16) >= d.thresh16) ? d.scale : 0.f;
    f[s][2] = ((x[2 * s + 1] & 0xffffu) >= d.thresh16) ? d.scale : 0.f;
    f[s][3] = ((x[2 * s + 1] >> 16) >= d.thresh16) ? d.scale : 0.f;
  }
}

template <int NSEG, bool VEC>
__global__ __launch_bounds__(256) void fuse_fwd_kernel(FuseArgs p) {
  const DropDev d = drop_resolve(p.drop);
  const int r = blockIdx.y;
  const int c0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (c0 >= p.P) return;
  const int64_t W = (int64_t)NSEG * p.P;
  const float* ar = p.a + (int64_t)r * p.lda;
  const float* br = p.b + (int64_t)r * p.ldb;
  float* orow = p.out + (int64_t)r * p.ldo;
  if (VEC) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(ar + c0);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(br + c0);
    float f[NSEG][4];
    fuse_factors<NSEG>(d, W, p.P, r, c0, f);
    f32x4 o[NSEG];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[0][j] = fuse_keep(av[j], f[0][j]);
      o[1][j] = fuse_keep(bv[j], f[1][j]);
      if (NSEG == 4) {
        o[2][j] = fuse_keep(bv[j] - av[j], f[2][j]);
        o[3][j] = fuse_keep(bv[j] * av[j], f[3][j]);
      }
    }
#pragma unroll
    for (int s = 0; s < NSEG; ++s) *reinterpret_cast<f32x4*>(orow + (int64_t)s * p.P + c0) = o[s];
  } else {
    for (int c = c0; c < min(c0 + 4, p.P); ++c) {
      const float a = ar[c], b = br[c];
      const uint64_t e = (uint64_t)r * (uint64_t)W + (uint64_t)c;
      orow[c] = drop_apply(d, e, a);
      orow[(int64_t)p.P + c] = drop_apply(d, e + (uint64_t)p.P, b);
      if (NSEG == 4) {
        orow[2 * (int64_t)p.P + c] = drop_apply(d, e + 2 * (uint64_t)p.P, b - a);
        orow[3 * (int64_t)p.P + c] = drop_apply(d, e + 3 * (uint64_t)p.P, b * a);
      }
    }
  }
}

// g_s = keep * scale * dout on segment s;  CAT2: da = g_0, db = g_1;  PAIR4: da = g_0 - g_2 + g_3 b, db = g_1 + g_2 + g_3 a
template <int NSEG, bool VEC>
__global__ __launch_bounds__(256) void fuse_bwd_kernel(FuseArgs p) {
  const DropDev d = drop_resolve(p.drop);
  const int r = blockIdx.y;
  const int c0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (c0 >= p.P) return;
  const int64_t W = (int64_t)NSEG * p.P;
  const float* drow = p.dout + (int64_t)r * p.ldd;
  float* dar = p.da + (int64_t)r * p.ldda;
  float* dbr = p.db + (int64_t)r * p.lddb;
  if (VEC) {
    f32x4 g[NSEG];
#pragma unroll
    for (int s = 0; s < NSEG; ++s) g[s] = *reinterpret_cast<const f32x4*>(drow + (int64_t)s * p.P + c0);
    f32x4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
    if (NSEG == 4) {
      av = *reinterpret_cast<const f32x4*>(p.a + (int64_t)r * p.lda + c0);
      bv = *reinterpret_cast<const f32x4*>(p.b + (int64_t)r * p.ldb + c0);
    }
    float f[NSEG][4];
    fuse_factors<NSEG>(d, W, p.P, r, c0, f);
    f32x4 da, db;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float g0 = fuse_keep(g[0][j], f[0][j]), g1 = fuse_keep(g[1][j], f[1][j]);
      if (NSEG == 4) {
        const float g2 = fuse_keep(g[2][j], f[2][j]), g3 = fuse_keep(g[3][j], f[3][j]);
        da[j] = (g0 - g2) + g3 * bv[j];
        db[j] = (g1 + g2) + g3 * av[j];
      } else {
        da[j] = g0;
        db[j] = g1;
      }
    }
    *reinterpret_cast<f32x4*>(dar + c0) = da;
    *reinterpret_cast<f32x4*>(dbr + c0) = db;
  } else {
    for (int c = c0; c < min(c0 + 4, p.P); ++c) {
      const uint64_t e = (uint64_t)r * (uint64_t)W + (uint64_t)c;
      const float g0 = drop_apply(d, e, drow[c]);
      const float g1 = drop_apply(d, e + (uint64_t)p.P, drow[(int64_t)p.P + c]);
      if (NSEG == 4) {
        const float a = p.a[(int64_t)r * p.lda + c], b = p.b[(int64_t)r * p.ldb + c];
        const float g2 = drop_apply(d, e + 2 * (uint64_t)p.P, drow[2 * (int64_t)p.P + c]);
        const float g3 = drop_apply(d, e + 3 * (uint64_t)p.P, drow[3 * (int64_t)p.P + c]);
        dar[c] = (g0 - g2) + g3 * b;
        dbr[c] = (g1 + g2) + g3 * a;
      } else {
        dar[c] = g0;
        dbr[c] = g1;
      }
    }
  }
}

// du[i] = y[i] > 0 ? dy[i] : 0
template <bool VEC>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* dy, const float* y, float* du, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n4; i += stride) {
      const f32x4 g = reinterpret_cast<const f32x4*>(dy)[i], v = reinterpret_cast<const f32x4*>(y)[i];
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = v[j] > 0.f ? g[j] : 0.f;
      reinterpret_cast<f32x4*>(du)[i] = o;
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += stride) du[i] = y[i] > 0.f ? dy[i] : 0.f;
  } else {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += stride) du[i] = y[i] > 0.f ? dy[i] : 0.f;
  }
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// shared argument checks of the two feature calls: -> 0, or the status after mvptr_set_error
int fuse_check(const char* name, int rows, int P, int mode) {
  if (rows < 1 || P < 1) MVPTR_FAIL(MVPTR_BAD_SHAPE, "%s: rows and P must be >= 1 (got %d, %d)", name, rows, P);
  if (mode != MVPTR_FUSE_CAT2 && mode != MVPTR_FUSE_PAIR4) MVPTR_FAIL(MVPTR_BAD_SHAPE, "%s: unknown mode %d", name, mode);
  if (rows > 65535) MVPTR_FAIL(MVPTR_BAD_SHAPE, "%s: at most 65535 rows per call (got %d)", name, rows);
  const int nseg = mode == MVPTR_FUSE_PAIR4 ? 4 : 2;
  if (P > (1 << 28) || (int64_t)rows * nseg * P >= ((int64_t)1 << 33))
    MVPTR_FAIL(MVPTR_BAD_SHAPE, "%s: rows * W must stay below 2^33 (rows %d, P %d)", name, rows, P);
  return MVPTR_OK;
}

}  // namespace

extern "C" int mvptr_fuse_features_fwd(const float* a, int64_t lda, const float* b, int64_t ldb, int rows, int P, int mode,
                                       const mvptr_dropout* drop, float* out, int64_t ldo, void* stream) {
  if (const int rc = fuse_check("fuse_features_fwd", rows, P, mode)) return rc;
  const int nseg = mode == MVPTR_FUSE_PAIR4 ? 4 : 2;
  if (!a || !b || !out) MVPTR_FAIL(MVPTR_BAD_SHAPE, "fuse_features_fwd: NULL argument");
  if (lda < P || ldb < P || ldo < (int64_t)nseg * P)
    MVPTR_FAIL(MVPTR_BAD_SHAPE, "fuse_features_fwd: a row stride is shorter than its row (lda %lld, ldb %lld, ldo %lld, P %d)",
               (long long)lda, (long long)ldb, (long long)ldo, P);
  FuseArgs p = {};
  p.a = a; p.b = b; p.out = out;
  p.lda = lda; p.ldb = ldb; p.ldo = ldo;
  p.rows = rows; p.P = P; p.nseg = nseg;
  p.drop = make_dropdev(drop);
  const bool vec = (P % 4 == 0) && (lda % 4 == 0) && (ldb % 4 == 0) && (ldo % 4 == 0) && aligned16(a) && aligned16(b) && aligned16(out);
  const dim3 grid((P + 1023) / 1024, rows);
  const hipStream_t s = (hipStream_t)stream;
  if (nseg == 4) {
    if (vec) hipLaunchKernelGGL((fuse_fwd_kernel<4, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fuse_fwd_kernel<4, false>), grid, dim3(256), 0, s, p);
  } else {
    if (vec) hipLaunchKernelGGL((fuse_fwd_kernel<2, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fuse_fwd_kernel<2, false>), grid, dim3(256), 0, s, p);
  }
  MVPTR_CHECK_LAUNCH("fuse_features_fwd");
  return MVPTR_OK;
}

extern "C" int mvptr_fuse_features_bwd(const float* a, int64_t lda, const float* b, int64_t ldb, const float* dout, int64_t ldd, int rows,
                                       int P, int mode, const mvptr_dropout* drop, float* da, int64_t ldda, float* db, int64_t lddb,
                                       void* stream) {
  if (const int rc = fuse_check("fuse_features_bwd", rows, P, mode)) return rc;
  const int nseg = mode == MVPTR_FUSE_PAIR4 ? 4 : 2;
  if (!a || !b || !dout || !da || !db) MVPTR_FAIL(MVPTR_BAD_SHAPE, "fuse_features_bwd: NULL argument");
  if (lda < P || ldb < P || ldda < P || lddb < P || ldd < (int64_t)nseg * P)
    MVPTR_FAIL(MVPTR_BAD_SHAPE, "fuse_features_bwd: a row stride is shorter than its row (lda %lld, ldb %lld, ldd %lld, ldda %lld, lddb %lld, P %d)",
               (long long)lda, (long long)ldb, (long long)ldd, (long long)ldda, (long long)lddb, P);
  FuseArgs p = {};
  p.a = a; p.b = b; p.dout = dout; p.da = da; p.db = db;
  p.lda = lda; p.ldb = ldb; p.ldd = ldd; p.ldda = ldda; p.lddb = lddb;
  p.rows = rows; p.P = P; p.nseg = nseg;
  p.drop = make_dropdev(drop);
  const bool vec = (P % 4 == 0) && (lda % 4 == 0) && (ldb % 4 == 0) && (ldd % 4 == 0) && (ldda % 4 == 0) && (lddb % 4 == 0) &&
                   aligned16(a) && aligned16(b) && aligned16(dout) && aligned16(da) && aligned16(db);
  const dim3 grid((P + 1023) / 1024, rows);
  const hipStream_t s = (hipStream_t)stream;
  if (nseg == 4) {
    if (vec) hipLaunchKernelGGL((fuse_bwd_kernel<4, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fuse_bwd_kernel<4, false>), grid, dim3(256), 0, s, p);
  } else {
    if (vec) hipLaunchKernelGGL((fuse_bwd_kernel<2, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fuse_bwd_kernel<2, false>), grid, dim3(256), 0, s, p);
  }
  MVPTR_CHECK_LAUNCH("fuse_features_bwd");
  return MVPTR_OK;
}

extern "C" int mvptr_relu_bwd(const float* dy, const float* y, float* du, int64_t n, void* stream) {
  if (n < 1) MVPTR_FAIL(MVPTR_BAD_SHAPE, "relu_bwd: n must be >= 1");
  if (!dy || !y || !du) MVPTR_FAIL(MVPTR_BAD_SHAPE, "relu_bwd: NULL argument");
  const bool vec = aligned16(dy) && aligned16(y) && aligned16(du);
  const int64_t work = vec ? (n + 3) / 4 : n;
  int grid = (int)((work + 255) / 256);
  if (grid > 2048) grid = 2048;
  if (vec) hipLaunchKernelGGL((relu_bwd_kernel<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, dy, y, du, n);
  else hipLaunchKernelGGL((relu_bwd_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, dy, y, du, n);
  MVPTR_CHECK_LAUNCH("relu_bwd");
  return MVPTR_OK;
}
