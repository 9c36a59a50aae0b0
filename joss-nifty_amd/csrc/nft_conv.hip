// Periodic convolution with a real, even harmonic-space kernel for gfx950.
//
// Replaces FuncConvolutionOperator of the reference
// (src/operators/convolution_operators.py, RGSpace.get_conv_kernel_from_func
// in src/domains/rg_space.py):  C x = Re ifftn(kt * fftn(x)) with kt the
// kernel's harmonic-space values and kt[0] = 1.  kt is real and even, so the
// whole convolution runs on the half complex spectrum of the R2C row pass:
//   1. R2C rows along the last axis (existing pass, colscale in its prologue)
//   2. 3-D: forward C2C over the middle axis (existing strided pass)
//   3. column sandwich over axis 0: a tile of L adjacent columns is loaded to
//      LDS once, transformed, multiplied by the kt / N table, transformed back
//      and stored -- no spectrum round trip through HBM in between.  Axes of
//      1024 and more run the four-step split N = N1 * N2: the existing pass A
//      (N1-point FFTs, twiddle), the sandwich over the N2-point pass B (which
//      also applies the conjugate twiddle on its way out), pass A inverted.
//   4. 3-D: inverse C2C over the middle axis
//   5. C2R rows: two half spectra packed as one complex line by their
//      Hermitian symmetry, one inverse FFT, real part -> row 2l, imaginary
//      part -> row 2l + 1; scale * rowscale and the quadratic-form partials
//      in the epilogue.
// fp64 only.  No atomics, no device-global state, no host synchronisation or
// allocation: capturable in a HIP graph.  Every line is transformed by the
// same arithmetic whatever tile it lands in, and the C2R tiles never straddle
// two vectors, so vector v of a batched call is bitwise the single call.
//
// nft_conv_space_*: the same operator on space 0 of a two-space domain, three
// passes over the data with the global-mean term of the reference's product
// domain form (see "sub-space passes" below).
#include <cstdint>
#include <cstring>

#include "fast_dispatch.hpp"
#include "nft_api_internal.hpp"

namespace nft {
namespace conv {

using namespace fast;
using C = double2;

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ------------------------------------------------------------ column sandwich
struct SandArgs {
  Lines g;              // in place: the out_* strides are not used
  C* buf;
  const C* tw;          // length-N table exp(-2 pi i k / N)
  const C* tw2;         // four-step twiddle table of length Nfull (or null)
  const double* table;  // kt / Npix, [n_axis][I]
  int km, kx, Nfull;    // full-axis index k = m * km + x * kx
  // table index mode: inner == 0: [k][column]; inner >= 1 (sub-space
  // convolution): [k][column / inner], tcols = I / inner table columns, the
  // table broadcast over the `inner` adjacent columns of one pixel
  int inner;
  long long tcols;
};

template <int N, int NT, int VP>
__global__ __launch_bounds__(NT) void sandwich_kernel(SandArgs a) {
  constexpr int L = NT * VP / N;
  static_assert(L >= 1, "NT*VP must cover one line");
  constexpr int PITCH = pass_pitch<N, false>();
  constexpr int PS = pass_pad<N, false>();
  constexpr int SHL = ilog2(L);
  extern __shared__ __align__(16) unsigned char smem[];
  C* lds = (C*)smem;
  C* twq = (C*)(smem + tw_lds_offset<double, N, NT, K_C2C, false, VP>());
  const int tid = threadIdx.x;
  for (int r = tid; r < N / 4; r += NT) twq[r] = a.tw[r];  // synced before the first stage
  const Lines& g = a.g;
  const Tile tl = strided_tile<L>(g, (long long)blockIdx.x, 0);
  const long long base = tl.o * g.in_so + tl.m * g.in_sm;
  const int m = (int)tl.m;
#pragma unroll
  for (int r = 0; r < VP; ++r) {
    const int e = tid + r * NT;
    const int x = e >> SHL, l = e & (L - 1);
    const long long li = tl.i0 + l;
    C v = C{0.0, 0.0};
    if (li < g.I) v = a.buf[base + li * g.in_si + (long long)x * g.in_sn];
    lds[l * PITCH + padx<PS>(x)] = v;
  }
  __syncthreads();
  fft<double, N, NT, L, PITCH, PS>(lds, twq, tid);
  // spectrum * table, conjugated for the inverse transform by a forward one;
  // every thread rewrites the slots it reads
#pragma unroll
  for (int r = 0; r < VP; ++r) {
    const int e = tid + r * NT;
    const int x = e >> SHL, l = e & (L - 1);
    const long long li = tl.i0 + l;
    const long long k = (long long)m * a.km + (long long)x * a.kx;
    double w = 0.0;
    if (li < g.I) w = a.inner ? a.table[k * a.tcols + (unsigned)li / (unsigned)a.inner] : a.table[k * g.I + li];
    const C v = lds[l * PITCH + padx<PS>(x)];
    lds[l * PITCH + padx<PS>(x)] = C{v.x * w, -(v.y * w)};
  }
  __syncthreads();
  fft<double, N, NT, L, PITCH, PS>(lds, twq, tid);
#pragma unroll
  for (int r = 0; r < VP; ++r) {
    const int e = tid + r * NT;
    const int x = e >> SHL, l = e & (L - 1);
    const long long li = tl.i0 + l;
    C v = lds[l * PITCH + padx<PS>(x)];
    v.y = -v.y;
    if (a.tw2) v = cmul(v, cconj(a.tw2[(m * x) & (a.Nfull - 1)]));
    if (li < g.I) a.buf[base + li * g.in_si + (long long)x * g.in_sn] = v;
  }
}

template <int N>
static int launch_sandwich_n(const SandArgs& a, hipStream_t s) {
  constexpr int NT = nt_strided_launch<double>(N);
  constexpr int VP = vp_strided<double>(N);
  constexpr int L = NT * VP / N;
  const size_t lds = pass_lds_bytes<double, N, NT, K_C2C, false, VP>();
  const long long ntiles = a.g.O * a.g.M * ((a.g.I + L - 1) / L);
  if (ntiles <= 0) return NFT_OK;
  if (ntiles > 0x7fffffffLL) {
    set_last_error("conv: too many tiles");
    return NFT_ERR_UNSUPPORTED;
  }
  if (lds > 65536) {
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute((const void*)sandwich_kernel<N, NT, VP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
      attr_set = true;
    }
  }
  prof_mark(s, "conv_sandwich");
  hipLaunchKernelGGL((sandwich_kernel<N, NT, VP>), dim3((unsigned)ntiles), dim3(NT), lds, s, a);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

static int launch_sandwich(int N, SandArgs& a, hipStream_t s) {
  const void* tw = nullptr;
  int st = get_twiddles(N, 0, &tw);
  if (st != NFT_OK) return st;
  a.tw = (const C*)tw;
  switch (N) {
    case 8: return launch_sandwich_n<8>(a, s);
    case 16: return launch_sandwich_n<16>(a, s);
    case 32: return launch_sandwich_n<32>(a, s);
    case 64: return launch_sandwich_n<64>(a, s);
    case 128: return launch_sandwich_n<128>(a, s);
    case 256: return launch_sandwich_n<256>(a, s);
    case 512: return launch_sandwich_n<512>(a, s);
  }
  set_last_error("conv sandwich: unsupported length %d", N);
  return NFT_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------ C2R row pass
struct C2RArgs {
  const C* spec;  // [nvec][rows][N / 2 + 1]
  const C* tw;
  double* y;
  long long ys;
  const double* rowscale;  // [rows * N] or null
  double scale;
  long long rows;  // real rows per vector (even)
  int tpi;         // tiles per vector
  double* qpart;
  long long qstride;
};

template <int N, int NT>
__global__ __launch_bounds__(NT) void c2r_kernel(C2RArgs a) {
  constexpr int L = NT * VPT / N;
  static_assert(L >= 1, "NT*VPT must cover one line");
  constexpr int PITCH = pass_pitch<N, true>();
  constexpr int SHN = ilog2(N);
  constexpr int NH = N / 2 + 1;
  extern __shared__ __align__(16) unsigned char smem[];
  C* lds = (C*)smem;
  C* twq = (C*)(smem + tw_lds_offset<double, N, NT, K_C2C, true>());
  const int tid = threadIdx.x;
  for (int r = tid; r < N / 4; r += NT) twq[r] = a.tw[r];  // synced before the first stage
  const long long item = (long long)blockIdx.x / a.tpi;
  const int tt = (int)((long long)blockIdx.x - item * a.tpi);
  const long long pl0 = (long long)tt * L;  // first pair-line of the tile within the vector
  const long long npl = a.rows >> 1;
  // Z = A + i B from the half spectra A (row 2l) and B (row 2l + 1):
  // Z[k] = A[k] + i B[k], Z[N - k] = conj(A[k]) + i conj(B[k]); stored
  // conjugated (the inverse transform runs as a forward one).  The imaginary
  // parts of A and B at k = 0 and k = N / 2 are rounding residue of the
  // other axes' passes and are dropped, as any C2R transform drops them.
  for (int e = tid; e < L * NH; e += NT) {
    const int l = e / NH;
    const int k = e - l * NH;
    const long long pl = pl0 + l;
    C A = C{0.0, 0.0}, B = C{0.0, 0.0};
    if (pl < npl) {
      const long long r0 = (item * a.rows + 2 * pl) * NH + k;
      A = a.spec[r0];
      B = a.spec[r0 + NH];
    }
    if (k == 0 || k == N / 2) {
      lds[l * PITCH + k] = C{A.x, -B.x};
    } else {
      lds[l * PITCH + k] = C{A.x - B.y, -(A.y + B.x)};
      lds[l * PITCH + N - k] = C{A.x + B.y, A.y - B.x};
    }
  }
  __syncthreads();
  fft<double, N, NT, L, PITCH, -1>(lds, twq, tid);
  double qs = 0.0;
#pragma unroll
  for (int r = 0; r < VPT; ++r) {
    const int e = tid + r * NT;
    const int l = e >> SHN;
    const int x = e & (N - 1);
    const long long pl = pl0 + l;
    if (pl >= npl) continue;
    const C w = lds[l * PITCH + x];
    const double t0 = w.x, t1 = -w.y;
    const long long j0 = 2 * pl * N + x;
    double s0 = a.scale, s1 = a.scale;
    if (a.rowscale) {
      s0 *= a.rowscale[j0];
      s1 *= a.rowscale[j0 + N];
    }
    const double y0 = s0 * t0, y1 = s1 * t1;
    a.y[item * a.ys + j0] = y0;
    a.y[item * a.ys + j0 + N] = y1;
    qs += t0 * y0;
    qs += t1 * y1;
  }
  if (a.qpart) {
    // fixed-order block sum (wave shuffle trees, then the waves in order),
    // as the quadratic-form epilogue of the unpack pass; the line buffer is
    // free once every wave has read its values
    __syncthreads();
    double* qsh = (double*)smem;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) qs += __shfl_down(qs, off, 64);
    if ((tid & 63) == 0) qsh[tid >> 6] = qs;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int w = 0; w < NT / 64; ++w) s += qsh[w];
      a.qpart[item * a.qstride + tt] = s;
    }
  }
}

template <int N>
static int launch_c2r_n(const C2RArgs& a, int nvec, hipStream_t s) {
  constexpr int NT = nt_rows(N);
  const size_t lds = pass_lds_bytes<double, N, NT, K_C2C, true>();
  const long long ntiles = (long long)nvec * a.tpi;
  if (ntiles <= 0) return NFT_OK;
  if (ntiles > 0x7fffffffLL) {
    set_last_error("conv: too many tiles");
    return NFT_ERR_UNSUPPORTED;
  }
  if (lds > 65536) {
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute((const void*)c2r_kernel<N, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
      attr_set = true;
    }
  }
  prof_mark(s, a.qpart ? "conv_c2r+quad" : "conv_c2r");
  hipLaunchKernelGGL((c2r_kernel<N, NT>), dim3((unsigned)ntiles), dim3(NT), lds, s, a);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

static int launch_c2r(int N, C2RArgs& a, int nvec, hipStream_t s) {
  const void* tw = nullptr;
  int st = get_twiddles(N, 0, &tw);
  if (st != NFT_OK) return st;
  a.tw = (const C*)tw;
#define NFT_CASE(n) \
  case n: return launch_c2r_n<n>(a, nvec, s);
  switch (N) {
    NFT_CASE(8) NFT_CASE(16) NFT_CASE(32) NFT_CASE(64) NFT_CASE(128) NFT_CASE(256) NFT_CASE(512)
    NFT_CASE(1024) NFT_CASE(2048) NFT_CASE(4096) NFT_CASE(8192)
  }
#undef NFT_CASE
  set_last_error("conv C2R: unsupported length %d", N);
  return NFT_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------ existing passes
// launched through nft_fft.hip (fast_pass_f64): the engine's kernels stay
// instantiated in that one translation unit, so the transforms run the very
// code objects they run without this file
static int launch_r2c(int N, FastArgs<double>& a, hipStream_t s) { return fast_pass_f64(K_R2C, true, N, a, s); }

static int launch_c2c_strided(int N, FastArgs<double>& a, hipStream_t s) {
  return fast_pass_f64(K_C2C, false, N, a, s);
}

// ------------------------------------------------------------ sub-space passes
// Convolution over space 0 of a two-space domain (S = n0 x n1, X = ne pixels,
// ne even): the real array (n0, n1, ne) is read as complex (n0, n1, inner),
// inner = ne / 2, so slices 2j and 2j + 1 of X travel as real and imaginary
// part through full-length C2C transforms over axes 1 and 0 and a REAL table.
//   1. axis-1 forward pass: colscale and the vector stride in the prologue,
//      per-tile sums of the k1 = 0 outputs (the line sums) for the mean
//   2. mean fold: cmean[v] = (1 - k0) * mean(colscale * x[v])
//   3. the column sandwich over axis 0, table indexed [k0][k1]
//   4. axis-1 inverse pass: t = value + cmean[v], y = scale * rowscale * t,
//      per-tile partials of t . y
// A line of the axis-1 passes is (r0, i): elements (r0, x, i), x < n1, at
// complex offset (r0 * n1 + x) * inner + i.  The lines of one vector are
// numbered q = r0 * inner + i and tiled L at a time over q, so a tile spans
// several r0 where inner < L (no idle lanes) and never two vectors.
struct SpaceArgs {
  const double* x;  // forward: input vectors
  long long xs;
  const double* colscale;
  C* buf;  // [nvec][n0][n1][inner]
  const C* tw;
  double* y;  // inverse: output vectors
  long long ys;
  const double* rowscale;
  double scale;
  const double* cmean;  // inverse: [nvec]
  double* part;         // forward: mean partials; inverse: qpart (or null)
  long long pstride;
  long long lines;  // n0 * inner lines per vector
  int inner, tpv;   // tiles per vector
  int al;           // x / colscale (y / rowscale) allow 16-byte accesses
};

constexpr int SP_NT = 256;
constexpr int sp_lines(int N) { return SP_NT * VPT / N; }
static size_t sp_lds_align(size_t b) { return (b + 15) & ~(size_t)15; }

__device__ __forceinline__ C ld2(const double* p, int al) {
  if (al) return *(const C*)p;
  return C{p[0], p[1]};
}

// fixed-order block sum: wave shuffle trees, then the waves in order (as
// c2r_kernel); the result is valid in thread 0.  sh: NT / 64 doubles of LDS
// free for use (synced here before it is written)
template <int NT>
__device__ __forceinline__ double block_sum(double s, double* sh, int tid) {
  __syncthreads();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((tid & 63) == 0) sh[tid >> 6] = s;
  __syncthreads();
  double r = 0.0;
  if (tid == 0)
    for (int w = 0; w < NT / 64; ++w) r += sh[w];
  return r;
}

template <int N, bool INV>
__global__ __launch_bounds__(SP_NT) void space_axis1_kernel(SpaceArgs a) {
  constexpr int NT = SP_NT;
  constexpr int L = sp_lines(N);
  static_assert(L >= 1 && NT % L == 0, "a thread keeps one line through the load and store loops");
  constexpr int PITCH = pass_pitch<N, false>();
  constexpr int PS = pass_pad<N, false>();
  constexpr int SHL = ilog2(L);
  constexpr int XS = NT / L;  // x step between a thread's values
  extern __shared__ __align__(16) unsigned char smem[];
  C* lds = (C*)smem;
  C* twq = (C*)(smem + (((size_t)L * PITCH * sizeof(C) + 15) & ~(size_t)15));
  const int tid = threadIdx.x;
  for (int r = tid; r < N / 4; r += NT) twq[r] = a.tw[r];  // synced before the first stage
  const long long item = (long long)blockIdx.x / a.tpv;
  const int tt = (int)((long long)blockIdx.x - item * a.tpv);
  const int l = tid & (L - 1);
  const int x0 = tid >> SHL;
  const long long q = (long long)tt * L + l;
  const bool live = q < a.lines;
  const unsigned r0 = live ? (unsigned)q / (unsigned)a.inner : 0u;
  const unsigned i = live ? (unsigned)q - r0 * (unsigned)a.inner : 0u;
  const long long off0 = (long long)r0 * N * a.inner + i;  // complex offset of element x = 0
  const long long P2 = a.lines * N;                        // complex values per vector
  C* buf = a.buf + item * P2;
#pragma unroll
  for (int r = 0; r < VPT; ++r) {
    const int x = x0 + r * XS;
    const long long off = off0 + (long long)x * a.inner;
    C v = C{0.0, 0.0};
    if (live) {
      if constexpr (INV) {
        v = buf[off];
        v.y = -v.y;
      } else {
        v = ld2(a.x + item * a.xs + 2 * off, a.al);
        if (a.colscale) {
          const C c = ld2(a.colscale + 2 * off, a.al);
          v.x *= c.x;
          v.y *= c.y;
        }
      }
    }
    lds[l * PITCH + padx<PS>(x)] = v;
  }
  __syncthreads();
  fft<double, N, NT, L, PITCH, PS>(lds, twq, tid);
  double s = 0.0;
  if constexpr (!INV) {
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
      const int x = x0 + r * XS;
      const C w = lds[l * PITCH + padx<PS>(x)];
      if (live) {
        buf[off0 + (long long)x * a.inner] = w;
        if (x == 0) s = w.x + w.y;  // the line's sum, both slices
      }
    }
    const double tot = block_sum<NT>(s, (double*)smem, tid);
    if (tid == 0) a.part[item * a.pstride + tt] = tot;
  } else {
    const double cm = a.cmean[item];
    double* y = a.y + item * a.ys;
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
      const int x = x0 + r * XS;
      const C w = lds[l * PITCH + padx<PS>(x)];
      if (!live) continue;
      const long long off = off0 + (long long)x * a.inner;
      const double t0 = w.x + cm, t1 = -w.y + cm;
      double s0 = a.scale, s1 = a.scale;
      if (a.rowscale) {
        const C c = ld2(a.rowscale + 2 * off, a.al);
        s0 *= c.x;
        s1 *= c.y;
      }
      const double y0 = s0 * t0, y1 = s1 * t1;
      if (a.al) {
        *(C*)(y + 2 * off) = C{y0, y1};
      } else {
        y[2 * off] = y0;
        y[2 * off + 1] = y1;
      }
      s += t0 * y0;
      s += t1 * y1;
    }
    if (a.part) {
      const double tot = block_sum<NT>(s, (double*)smem, tid);
      if (tid == 0) a.part[item * a.pstride + tt] = tot;
    }
  }
}

// cmean[v] = coef * (the sum of vector v's tpv partials): thread t sums the
// partials t, t + NT, ... in index order, then the fixed-order block sum --
// an order set by tpv (the plan) alone
__global__ __launch_bounds__(SP_NT) void space_mean_kernel(const double* part, long long pstride, int tpv, double coef,
                                                           double* cmean) {
  __shared__ double sh[SP_NT / 64];
  const int tid = threadIdx.x;
  const double* p = part + (long long)blockIdx.x * pstride;
  double s = 0.0;
  for (int j = tid; j < tpv; j += SP_NT) s += p[j];
  const double tot = block_sum<SP_NT>(s, sh, tid);
  if (tid == 0) cmean[blockIdx.x] = coef * tot;
}

template <int N, bool INV>
static int launch_space_axis1_n(const SpaceArgs& a, int nvec, hipStream_t s) {
  constexpr int L = sp_lines(N);
  const size_t lds = sp_lds_align((size_t)L * pass_pitch<N, false>() * sizeof(C)) + (size_t)(N / 4) * sizeof(C);
  static_assert((size_t)L * pass_pitch<N, false>() * sizeof(C) + (N / 4) * sizeof(C) + 16 <= 65536, "LDS");
  const long long ntiles = (long long)nvec * a.tpv;
  if (ntiles <= 0) return NFT_OK;
  if (ntiles > 0x7fffffffLL) {
    set_last_error("conv: too many tiles");
    return NFT_ERR_UNSUPPORTED;
  }
  prof_mark(s, INV ? (a.part ? "conv_space_inv+quad" : "conv_space_inv") : "conv_space_fwd");
  hipLaunchKernelGGL((space_axis1_kernel<N, INV>), dim3((unsigned)ntiles), dim3(SP_NT), lds, s, a);
  NFT_HIP_CHECK(hipGetLastError());
  return NFT_OK;
}

template <bool INV>
static int launch_space_axis1(int N, SpaceArgs& a, int nvec, hipStream_t s) {
  const void* tw = nullptr;
  int st = get_twiddles(N, 0, &tw);
  if (st != NFT_OK) return st;
  a.tw = (const C*)tw;
#define NFT_CASE(n) \
  case n: return launch_space_axis1_n<n, INV>(a, nvec, s);
  switch (N) { NFT_CASE(8) NFT_CASE(16) NFT_CASE(32) NFT_CASE(64) NFT_CASE(128) NFT_CASE(256) NFT_CASE(512) }
#undef NFT_CASE
  set_last_error("conv space: unsupported axis-1 length %d", N);
  return NFT_ERR_UNSUPPORTED;
}

static bool space_plan_ok(const nft_conv_space_plan* p) {
  return p && p->n0 >= 1 && p->n1 >= 1 && p->inner >= 1 && p->table;
}

static bool space_ok(int64_t n0, int64_t n1, int64_t ne, int dtype) {
  if (dtype != 0 || n0 < 1 || n1 < 1 || ne < 2 || (ne & 1)) return false;
  if (n0 > 16384 || n1 > 512 || ne >= 0x7fffffffLL) return false;
  if ((long long)n0 * n1 * ne >= 0x7fffffffLL) return false;
  if (!strided_supported((int)n1)) return false;
  return strided_supported((int)n0) || fourstep_supported((int)n0);
}

static int space_tiles(const nft_conv_space_plan* p) {
  const long long L = sp_lines((int)p->n1);
  return (int)((p->n0 * p->inner + L - 1) / L);
}

// ------------------------------------------------------------ plan checks
static bool plan_ok(const nft_conv_plan* p) {
  if (!p || p->ndim < 1 || p->ndim > 3 || !p->table) return false;
  for (int d = 0; d < p->ndim; ++d)
    if (p->shape[d] < 1) return false;
  return true;
}

static bool native_ok(int ndim, const int64_t* shape, int dtype) {
  if (dtype != 0 || !shape || ndim < 2 || ndim > 3) return false;
  long long tot = 1;
  for (int d = 0; d < ndim; ++d) {
    if (shape[d] < 1 || shape[d] > 16384) return false;
    tot *= shape[d];
  }
  if (tot >= 0x7fffffffLL) return false;
  if (!rows_supported((int)shape[ndim - 1])) return false;
  if (ndim == 3 && !strided_supported((int)shape[1])) return false;
  const int n0 = (int)shape[0];
  return strided_supported(n0) || fourstep_supported(n0);
}

}  // namespace conv
}  // namespace nft

using namespace nft;
using namespace nft::conv;

extern "C" {

int nft_conv_supported(int ndim, const int64_t* shape, int dtype) { return native_ok(ndim, shape, dtype) ? 1 : 0; }

size_t nft_conv_workspace(const nft_conv_plan* plan, int nvec) {
  if (!plan_ok(plan) || nvec < 1) return 0;
  size_t n = (size_t)nvec;
  for (int d = 0; d < plan->ndim - 1; ++d) n *= (size_t)plan->shape[d];
  n *= (size_t)(plan->shape[plan->ndim - 1] / 2 + 1);
  return align256(n * sizeof(C));
}

int nft_conv_quad_blocks(const nft_conv_plan* plan) {
  if (!plan_ok(plan) || !native_ok(plan->ndim, plan->shape, 0)) return 0;
  long long rows = 1;
  for (int d = 0; d < plan->ndim - 1; ++d) rows *= plan->shape[d];
  const int N = (int)plan->shape[plan->ndim - 1];
  const long long L = nt_rows(N) * VPT / N;
  return (int)((rows / 2 + L - 1) / L);
}

int nft_conv_apply_batched(const nft_conv_plan* plan, const void* x, int64_t x_stride, const void* colscale,
                           void* y, int64_t y_stride, const void* rowscale, double scale, int nvec, int dtype,
                           double* qpart, int64_t qstride, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (!plan_ok(plan)) {
    set_last_error("conv: bad plan (ndim 1..3, positive shape, table)");
    return NFT_ERR_ARG;
  }
  if (!x || !y || nvec < 1) {
    set_last_error("conv: NULL vector or nvec < 1");
    return NFT_ERR_ARG;
  }
  if (!native_ok(plan->ndim, plan->shape, dtype)) {
    set_last_error("conv: grid or dtype not served by the native pipeline (nft_conv_supported)");
    return NFT_ERR_UNSUPPORTED;
  }
  const int nd = plan->ndim;
  const int N = (int)plan->shape[nd - 1];
  const long long NH = N / 2 + 1;
  const int n0 = (int)plan->shape[0];
  const int n1 = nd == 3 ? (int)plan->shape[1] : 1;
  const long long rows = (long long)n0 * n1;
  const long long P = rows * N;
  if (x_stride < P || y_stride < P) {
    set_last_error("conv: vector strides shorter than a vector");
    return NFT_ERR_ARG;
  }
  const int nqb = nft_conv_quad_blocks(plan);
  if (qpart && qstride < nqb) {
    set_last_error("conv: qstride shorter than nft_conv_quad_blocks");
    return NFT_ERR_ARG;
  }
  const size_t need = nft_conv_workspace(plan, nvec);
  if (!ws || ws_bytes < need) {
    set_last_error("conv workspace too small (%zu < %zu)", ws_bytes, need);
    return NFT_ERR_ARG;
  }
  int st;
  {  // 1. R2C rows, colscale and the vector stride in the prologue
    FastArgs<double> a;
    memset(&a, 0, sizeof(a));
    a.in = x;
    a.out = ws;
    a.g.O = (long long)nvec * rows;
    a.g.M = a.g.I = 1;
    a.g.in_so = N;
    a.g.in_sn = 1;
    a.g.out_so = NH;
    a.g.out_sn = 1;
    a.Ireal = a.g.O;
    a.scale = 1.0;
    if (colscale || x_stride != P) {
      a.f.pro = 1;
      a.f.px = x;
      a.f.pa = colscale;
      a.f.P = P;
      a.f.pshift = -1;
      if (is_pow2(P)) {
        int sh = 0;
        while ((1LL << sh) < P) ++sh;
        a.f.pshift = sh;
      }
      a.f.nb = nvec;
      a.f.sx = x_stride;
      a.f.ce = 1;
    }
    if ((st = launch_r2c(N, a, stream)) != NFT_OK) return st;
  }
  const long long I0 = (long long)n1 * NH;  // columns of axis 0
  auto middle = [&](int inverse) -> int {   // 2. / 4. C2C over the middle axis, in place
    FastArgs<double> a;
    memset(&a, 0, sizeof(a));
    a.in = ws;
    a.out = ws;
    a.g.O = (long long)nvec * n0;
    a.g.M = 1;
    a.g.I = NH;
    a.g.in_so = a.g.out_so = NH * n1;
    a.g.in_si = a.g.out_si = 1;
    a.g.in_sn = a.g.out_sn = NH;
    a.conj_in = a.conj_out = inverse;
    a.scale = 1.0;
    return launch_c2c_strided(n1, a, stream);
  };
  if (nd == 3 && (st = middle(0)) != NFT_OK) return st;
  if (strided_supported(n0)) {  // 3. the whole column in one sandwich
    SandArgs a;
    memset(&a, 0, sizeof(a));
    a.buf = (C*)ws;
    a.g.O = nvec;
    a.g.M = 1;
    a.g.I = I0;
    a.g.in_so = I0 * n0;
    a.g.in_si = 1;
    a.g.in_sn = I0;
    a.table = plan->table;
    a.km = 0;
    a.kx = 1;
    a.Nfull = n0;
    if ((st = launch_sandwich(n0, a, stream)) != NFT_OK) return st;
  } else {
    int N1, N2;
    fourstep_split(n0, N1, N2);
    const void* twN = nullptr;
    if ((st = get_twiddles(n0, 0, &twN)) != NFT_OK) return st;
    auto pass_a = [&](int inverse) -> int {  // N1-point FFTs over rows n2 + N2 * j, in place
      FastArgs<double> a;
      memset(&a, 0, sizeof(a));
      a.in = ws;
      a.out = ws;
      a.g.O = nvec;
      a.g.M = N2;
      a.g.I = I0;
      a.g.in_so = a.g.out_so = I0 * n0;
      a.g.in_sm = a.g.out_sm = I0;
      a.g.in_si = a.g.out_si = 1;
      a.g.in_sn = a.g.out_sn = I0 * N2;
      a.tw2 = inverse ? nullptr : twN;  // the sandwich applies the conjugate twiddle
      a.Nfull = n0;
      a.conj_in = a.conj_out = inverse;
      a.scale = 1.0;
      return launch_c2c_strided(N1, a, stream);
    };
    if ((st = pass_a(0)) != NFT_OK) return st;
    SandArgs a;  // pass B and its inverse: rows N2 * k1 + n2, element k2 is k = k1 + N1 * k2
    memset(&a, 0, sizeof(a));
    a.buf = (C*)ws;
    a.g.O = nvec;
    a.g.M = N1;
    a.g.I = I0;
    a.g.in_so = I0 * n0;
    a.g.in_sm = I0 * N2;
    a.g.in_si = 1;
    a.g.in_sn = I0;
    a.table = plan->table;
    a.tw2 = (const C*)twN;
    a.km = 1;
    a.kx = N1;
    a.Nfull = n0;
    if ((st = launch_sandwich(N2, a, stream)) != NFT_OK) return st;
    if ((st = pass_a(1)) != NFT_OK) return st;
  }
  if (nd == 3 && (st = middle(1)) != NFT_OK) return st;
  {  // 5. C2R rows with the epilogue
    C2RArgs a;
    memset(&a, 0, sizeof(a));
    a.spec = (const C*)ws;
    a.y = (double*)y;
    a.ys = y_stride;
    a.rowscale = (const double*)rowscale;
    a.scale = scale;
    a.rows = rows;
    a.tpi = nqb;
    a.qpart = qpart;
    a.qstride = qstride;
    if ((st = launch_c2r(N, a, nvec, stream)) != NFT_OK) return st;
  }
  return NFT_OK;
}

// ------------------------------------------------------------ sub-space API
int nft_conv_space_supported(int64_t n0, int64_t n1, int64_t ne, int dtype) {
  return space_ok(n0, n1, ne, dtype) ? 1 : 0;
}

// workspace: the complex grids, then the mean partials, then the mean terms
static size_t space_ws_grid(const nft_conv_space_plan* p, int nvec) {
  return align256((size_t)nvec * (size_t)p->n0 * (size_t)p->n1 * (size_t)p->inner * sizeof(C));
}

size_t nft_conv_space_workspace(const nft_conv_space_plan* plan, int nvec) {
  if (!space_plan_ok(plan) || nvec < 1) return 0;
  if (plan->n1 > 512 || plan->n0 > 16384 || plan->inner >= 0x40000000LL) return 0;
  const size_t tpv = (size_t)space_tiles(plan);
  return space_ws_grid(plan, nvec) + align256((size_t)nvec * tpv * sizeof(double)) +
         align256((size_t)nvec * sizeof(double));
}

int nft_conv_space_quad_blocks(const nft_conv_space_plan* plan) {
  if (!space_plan_ok(plan) || !space_ok(plan->n0, plan->n1, 2 * plan->inner, 0)) return 0;
  return space_tiles(plan);
}

int nft_conv_space_apply_batched(const nft_conv_space_plan* plan, const void* x, int64_t x_stride,
                                 const void* colscale, void* y, int64_t y_stride, const void* rowscale, double scale,
                                 int nvec, int dtype, double* qpart, int64_t qstride, void* ws, size_t ws_bytes,
                                 hipStream_t stream) {
  if (!space_plan_ok(plan)) {
    set_last_error("conv space: bad plan (positive n0, n1, inner, table)");
    return NFT_ERR_ARG;
  }
  if (!x || !y || nvec < 1) {
    set_last_error("conv space: NULL vector or nvec < 1");
    return NFT_ERR_ARG;
  }
  if (plan->inner >= 0x40000000LL || !space_ok(plan->n0, plan->n1, 2 * plan->inner, dtype)) {
    set_last_error("conv space: domain or dtype not served by the native pipeline (nft_conv_space_supported)");
    return NFT_ERR_UNSUPPORTED;
  }
  const int n0 = (int)plan->n0, n1 = (int)plan->n1, inner = (int)plan->inner;
  const long long P = (long long)n0 * n1 * inner * 2;  // real pixels per vector
  if (x_stride < P || y_stride < P) {
    set_last_error("conv space: vector strides shorter than a vector");
    return NFT_ERR_ARG;
  }
  const int tpv = space_tiles(plan);
  if (qpart && qstride < tpv) {
    set_last_error("conv space: qstride shorter than nft_conv_space_quad_blocks");
    return NFT_ERR_ARG;
  }
  const size_t need = nft_conv_space_workspace(plan, nvec);
  if (!ws || ws_bytes < need) {
    set_last_error("conv space workspace too small (%zu < %zu)", ws_bytes, need);
    return NFT_ERR_ARG;
  }
  C* grid = (C*)ws;
  double* mpart = (double*)((char*)ws + space_ws_grid(plan, nvec));
  double* cmean = (double*)((char*)mpart + align256((size_t)nvec * (size_t)tpv * sizeof(double)));
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  int st;
  SpaceArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.buf = grid;
  sa.lines = (long long)n0 * inner;
  sa.inner = inner;
  sa.tpv = tpv;
  {  // 1. axis-1 forward pass, colscale and the vector stride in the prologue
    SpaceArgs a = sa;
    a.x = (const double*)x;
    a.xs = x_stride;
    a.colscale = (const double*)colscale;
    a.part = mpart;
    a.pstride = tpv;
    a.al = al16(x) && (x_stride & 1) == 0 && al16(colscale);
    if ((st = launch_space_axis1<false>(n1, a, nvec, stream)) != NFT_OK) return st;
  }
  // 2. the mean term of every vector
  prof_mark(stream, "conv_space_mean");
  hipLaunchKernelGGL(space_mean_kernel, dim3((unsigned)nvec), dim3(SP_NT), 0, stream, (const double*)mpart,
                     (long long)tpv, tpv, (1.0 - plan->gain0) / (double)P, cmean);
  NFT_HIP_CHECK(hipGetLastError());
  const long long I0 = (long long)n1 * inner;  // columns of axis 0
  if (strided_supported(n0)) {                 // 3. the whole column in one sandwich
    SandArgs a;
    memset(&a, 0, sizeof(a));
    a.buf = grid;
    a.g.O = nvec;
    a.g.M = 1;
    a.g.I = I0;
    a.g.in_so = I0 * n0;
    a.g.in_si = 1;
    a.g.in_sn = I0;
    a.table = plan->table;
    a.km = 0;
    a.kx = 1;
    a.Nfull = n0;
    a.inner = inner;
    a.tcols = n1;
    if ((st = launch_sandwich(n0, a, stream)) != NFT_OK) return st;
  } else {
    int N1, N2;
    fourstep_split(n0, N1, N2);
    const void* twN = nullptr;
    if ((st = get_twiddles(n0, 0, &twN)) != NFT_OK) return st;
    auto pass_a = [&](int inverse) -> int {  // N1-point FFTs over rows n2 + N2 * j, in place
      FastArgs<double> a;
      memset(&a, 0, sizeof(a));
      a.in = ws;
      a.out = ws;
      a.g.O = nvec;
      a.g.M = N2;
      a.g.I = I0;
      a.g.in_so = a.g.out_so = I0 * n0;
      a.g.in_sm = a.g.out_sm = I0;
      a.g.in_si = a.g.out_si = 1;
      a.g.in_sn = a.g.out_sn = I0 * N2;
      a.tw2 = inverse ? nullptr : twN;  // the sandwich applies the conjugate twiddle
      a.Nfull = n0;
      a.conj_in = a.conj_out = inverse;
      a.scale = 1.0;
      return launch_c2c_strided(N1, a, stream);
    };
    if ((st = pass_a(0)) != NFT_OK) return st;
    SandArgs a;  // pass B and its inverse: rows N2 * k1 + n2, element k2 is k = k1 + N1 * k2
    memset(&a, 0, sizeof(a));
    a.buf = grid;
    a.g.O = nvec;
    a.g.M = N1;
    a.g.I = I0;
    a.g.in_so = I0 * n0;
    a.g.in_sm = I0 * N2;
    a.g.in_si = 1;
    a.g.in_sn = I0;
    a.table = plan->table;
    a.tw2 = (const C*)twN;
    a.km = 1;
    a.kx = N1;
    a.Nfull = n0;
    a.inner = inner;
    a.tcols = n1;
    if ((st = launch_sandwich(N2, a, stream)) != NFT_OK) return st;
    if ((st = pass_a(1)) != NFT_OK) return st;
  }
  {  // 4. axis-1 inverse pass with the epilogue
    SpaceArgs a = sa;
    a.y = (double*)y;
    a.ys = y_stride;
    a.rowscale = (const double*)rowscale;
    a.scale = scale;
    a.cmean = cmean;
    a.part = qpart;
    a.pstride = qstride;
    a.al = al16(y) && (y_stride & 1) == 0 && al16(rowscale);
    if ((st = launch_space_axis1<true>(n1, a, nvec, stream)) != NFT_OK) return st;
  }
  return NFT_OK;
}

}  // extern "C"
