// The full-square step kernel family (step_kernel and its launch dispatch), shared by rbpf_kernels.hip -- which instantiates it for
// the built-in widths n_y = 1 and 3 -- and the rbpf_step_wide_*.hip units of the generic family's other widths.  gfx950 only.
#pragma once
#include "rbpf_internal.hpp"
#include "rbpf_device.hpp"
#include "rbpf_model_dev.hpp"

#ifndef RBPF_UC
#define RBPF_UC 8          // columns kept in flight per wave in the covariance stream
#endif
#ifndef RBPF_UC2
#define RBPF_UC2 4         // ... when a wave owns two row chunks per column
#endif
#ifndef RBPF_UC3
#define RBPF_UC3 2         // ... three row chunks
#endif
#ifndef RBPF_NT_LOAD
#define RBPF_NT_LOAD 0     // 1: nontemporal loads (defeats the Infinity-Cache reuse of sibling reads: keep 0)
#endif
#ifndef RBPF_NT_STORE
#define RBPF_NT_STORE 1    // 1: nontemporal stores of the streamed covariance
#endif

namespace rbpf {

typedef double dbl2 __attribute__((ext_vector_type(2)));

// Two consecutive rows of a stored covariance.  TS = double (the reference's precision) or float (fp32 STORAGE of the
// covariance banks, rbpf_options.storage = 1: half the HBM traffic; all arithmetic stays fp64).
typedef float flt2 __attribute__((ext_vector_type(2)));

template <typename TS> __device__ __forceinline__ dbl2 ld_pair(const TS* p);
template <> __device__ __forceinline__ dbl2 ld_pair<double>(const double* p) { return *reinterpret_cast<const dbl2*>(p); }
template <> __device__ __forceinline__ dbl2 ld_pair<float>(const float* p) {
  const flt2 v = *reinterpret_cast<const flt2*>(p);
  dbl2 o; o.x = (double)v.x; o.y = (double)v.y;
  return o;
}
template <typename TS> __device__ __forceinline__ void st_pair(TS* p, dbl2 v);
template <> __device__ __forceinline__ void st_pair<double>(double* p, dbl2 v) { *reinterpret_cast<dbl2*>(p) = v; }
template <> __device__ __forceinline__ void st_pair<float>(float* p, dbl2 v) {
  flt2 o; o.x = (float)v.x; o.y = (float)v.y;
  *reinterpret_cast<flt2*>(p) = o;
}

template <typename TS> struct Pair;                       // two stored rows as they sit in memory
template <> struct Pair<double> { typedef dbl2 type; };
template <> struct Pair<float> { typedef flt2 type; };
template <typename TS> __device__ __forceinline__ typename Pair<TS>::type ld_stream_raw(const TS* p) {
#if RBPF_NT_LOAD
  return __builtin_nontemporal_load(reinterpret_cast<const typename Pair<TS>::type*>(p));
#else
  return *reinterpret_cast<const typename Pair<TS>::type*>(p);
#endif
}

template <typename TS> __device__ __forceinline__ dbl2 ld_stream(const TS* p);
template <> __device__ __forceinline__ dbl2 ld_stream<double>(const double* p) {
#if RBPF_NT_LOAD
  return __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(p));
#else
  return *reinterpret_cast<const dbl2*>(p);
#endif
}
template <> __device__ __forceinline__ dbl2 ld_stream<float>(const float* p) {
#if RBPF_NT_LOAD
  const flt2 v = __builtin_nontemporal_load(reinterpret_cast<const flt2*>(p));
#else
  const flt2 v = *reinterpret_cast<const flt2*>(p);
#endif
  dbl2 o; o.x = (double)v.x; o.y = (double)v.y;
  return o;
}

template <typename TS> __device__ __forceinline__ void st_stream(TS* p, dbl2 v);
template <> __device__ __forceinline__ void st_stream<double>(double* p, dbl2 v) {
#if RBPF_NT_STORE
  __builtin_nontemporal_store(v, reinterpret_cast<dbl2*>(p));
#else
  *reinterpret_cast<dbl2*>(p) = v;
#endif
}
template <> __device__ __forceinline__ void st_stream<float>(float* p, dbl2 v) {
  flt2 o; o.x = (float)v.x; o.y = (float)v.y;
#if RBPF_NT_STORE
  __builtin_nontemporal_store(o, reinterpret_cast<flt2*>(p));
#else
  *reinterpret_cast<flt2*>(p) = o;
#endif
}

// ---------------------------------------------------------------------------------------------
// layout helpers (host + device)
// ---------------------------------------------------------------------------------------------
struct LdsPlan {
  int off_HK, off_xl, off_PHt, off_parts, off_tab, off_misc, off_red, off_kst, total;  // in doubles
};

__host__ __device__ inline int even_up(int x) { return (x + 1) & ~1; }

constexpr int kKBlock = 64;        // columns per stage of the blocked pending-factor buffer (KB variants of the step kernel)

// Epilogue scratch of the step kernel, sized from the measurement width d.  `misc`: 0..7 xn_new, 8..16 Rnb, then what thread 0
// broadcasts from phase E to phase F -- chol(S) | S | innovation | d spare doubles | the information form's qa, qb, sum(log diag).
// `red`: one row of NRED = d*d + d + 2e partial sums per wave.  At d <= 3 these are the fixed slots the kernel has always used
// (20 / 30 / 40 / 44, 64 doubles of misc, red rows of 16); wider models get what they need (d = 8: 168 and 4 x 82 doubles).
// lds_plan sizes the launch from the same functions the kernel indexes with.
__host__ __device__ constexpr int misc_cS(int) { return 20; }
__host__ __device__ constexpr int misc_SS(int d) { return d <= 3 ? 30 : 20 + d * d; }
__host__ __device__ constexpr int misc_e(int d) { return d <= 3 ? 40 : 20 + 2 * d * d; }
__host__ __device__ constexpr int misc_q(int d) { return d <= 3 ? 44 : 20 + 2 * d * d + 2 * d; }
__host__ __device__ constexpr int misc_doubles(int d) { return d <= 3 ? 64 : (misc_q(d) + 3 + 1) & ~1; }
__host__ __device__ constexpr int red_stride(int d, int e) { return d * d + d + 2 * e <= 16 ? 16 : (d * d + d + 2 * e + 1) & ~1; }

// R and R^-1 of the model: kernel arguments up to 3 x 3, device memory [R | R^-1] beyond (ModelDev::Rdev)
template <int D> __device__ __forceinline__ double model_R(const ModelDev& M, int q) {
  if constexpr (D <= 3) return M.R[q]; else return M.Rdev[q];
}
template <int D> __device__ __forceinline__ double model_Rinv(const ModelDev& M, int q) {
  if constexpr (D <= 3) return M.Rinv[q]; else return M.Rdev[D * D + q];
}

// Columns in flight per wave in the covariance stream, by row chunks per wave.  n_y = 4 and 5 keep half the columns of the other
// widths: measured at N_P = 8192, nLin = 256 (two chunks per wave, tools/generic_device_bench.py --ny), n_y = 4 takes 1.48 ms
// per step with 2 columns in flight against 1.68 ms with 4 -- two workgroups share a CU there and the accumulators
// acc[CPL][2][D+E] + ks[CPL][2][D] already fill the registers that leaves each -- while n_y = 6 and 8, whose LDS plan leaves one
// workgroup per CU, gain from 4 (2.14 against 2.40 ms, 2.28 against 2.53 ms).  No instantiation uses scratch memory either way
// (profiles/generic_ny_kernel_resources.txt).
#ifndef RBPF_UCW
#define RBPF_UCW 4
#endif
#ifndef RBPF_UCW2
#define RBPF_UCW2 2
#endif
#ifndef RBPF_UCW3
#define RBPF_UCW3 2
#endif
__host__ __device__ constexpr int step_uc(int d, int cpl) {
  return (d == 4 || d == 5) ? (cpl <= 1 ? RBPF_UCW : (cpl == 2 ? RBPF_UCW2 : RBPF_UCW3)) : (cpl <= 1 ? RBPF_UC : (cpl == 2 ? RBPF_UC2 : RBPF_UC3));
}

// kb != 0: the pending column factors K of the NS sets are NOT kept for all n columns (n * NS * D doubles: 74 KB at n = 1027,
// NS = 2, and 37 KB on top of the information form's 5 right-hand sides at n = 515 -- one workgroup per CU); they pass through a
// double-buffered stage of kKBlock columns instead, refilled while the previous block streams.  With one column phase
// (CS == 1) the per-phase partial sums are not needed either: the accumulators go straight to PHt.
__host__ __device__ inline LdsPlan lds_plan(int n, int d, int e, int ns, int ldx, int CS, int mc, int ktot, int kb = 0) {
  LdsPlan p;
  int o = 0;
  p.off_HK = o;    o += even_up(n * (d + e + (kb ? 0 : ns * d)));
  p.off_xl = o;    o += ldx;
  p.off_PHt = o;   o += (d + e) * ldx;
  p.off_parts = o; o += (kb && CS == 1) ? 0 : CS * (d + e) * mc;
  p.off_tab = o;   o += even_up(2 * (ktot > 0 ? ktot : 1));
  p.off_misc = o;  o += misc_doubles(d);
  p.off_red = o;   o += kWaves * red_stride(d, e);
  p.off_kst = o;   o += kb ? 2 * kKBlock * ns * d : 0;
  p.total = o;
  return p;
}

// ---------------------------------------------------------------------------------------------
// the streamed core block: lanes own rows (2 per 128-row chunk), waves walk columns.
// Per column the wave needs DE = D+E right-hand-side values (H rows, then the E extra vectors of the
// information form) and the D pending column factors; LDS record per column: [H(D) | X(E) | K(D)].
// ---------------------------------------------------------------------------------------------
template <int NSA>
struct SetPtrs { const double* p[NSA]; };

template <typename TS, int D, int E, int CPL, int UC, int NS, bool WR>
__device__ __forceinline__ void stream_core(const TS* __restrict__ src, TS* __restrict__ dst,
                                            const double* __restrict__ HK, const SetPtrs<(NS > 0 ? NS : 1)> KSrows,
                                            int ldx, int n, int nb, int mc, int chunk0, int chunk_stride, int CS,
                                            int wc, int lane, double* __restrict__ out_acc /* [D+E][mc] */) {
  // Every chunk handled here is valid (the caller decides wave-uniformly), so the loop body carries
  // no predicates: all UC*CPL loads of a round are issued back to back and stay in flight together.
  // NS pending rank-D factor sets are applied on the fly; WR = false (a "light" step of the multi-step
  // lazy update) only reads the base matrix.
  constexpr int DE = D + E, ND = NS * D, REC = DE + ND, NDA = ND > 0 ? ND : 1;
  double acc[CPL][2][DE];
  double ks[CPL][2][NDA];
  int r0[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    r0[q] = (chunk0 + q * chunk_stride) * kChunkRows + 2 * lane;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
      for (int k = 0; k < DE; ++k) acc[q][e][k] = 0.0;
#pragma unroll
      for (int sset = 0; sset < NS; ++sset)
#pragma unroll
        for (int k = 0; k < D; ++k) ks[q][e][sset * D + k] = KSrows.p[sset][(size_t)k * ldx + nb + r0[q] + e];
    }
  }
  const size_t colstep = (size_t)CS * mc;               // elements between two columns of this wave
  const TS* sp = src + (size_t)wc * mc;
  TS* dp = dst + (size_t)wc * mc;
  const double* hk = HK + (size_t)wc * REC;
  const int hkstep = CS * REC;

  int c = wc;
  for (; c + (UC - 1) * CS < n; c += UC * CS) {
    typename Pair<TS>::type v[UC][CPL];                 // kept in the stored type until used: float keeps half the registers
#pragma unroll
    for (int u = 0; u < UC; ++u)
#pragma unroll
      for (int q = 0; q < CPL; ++q) v[u][q] = ld_stream_raw<TS>(sp + u * colstep + r0[q]);
#pragma unroll
    for (int u = 0; u < UC; ++u) {
      double h[DE], kc[NDA];
#pragma unroll
      for (int k = 0; k < DE; ++k) h[k] = hk[u * hkstep + k];
#pragma unroll
      for (int k = 0; k < ND; ++k) kc[k] = hk[u * hkstep + DE + k];
#pragma unroll
      for (int q = 0; q < CPL; ++q) {
        double p0 = (double)v[u][q].x, p1 = (double)v[u][q].y;
#pragma unroll
        for (int k = 0; k < ND; ++k) { p0 = fma(-ks[q][0][k], kc[k], p0); p1 = fma(-ks[q][1][k], kc[k], p1); }
#pragma unroll
        for (int k = 0; k < DE; ++k) { acc[q][0][k] = fma(p0, h[k], acc[q][0][k]); acc[q][1][k] = fma(p1, h[k], acc[q][1][k]); }
        if (WR) { dbl2 o; o.x = p0; o.y = p1; st_stream(dp + u * colstep + r0[q], o); }
      }
    }
    sp += UC * colstep; dp += UC * colstep; hk += UC * hkstep;
  }
  for (; c < n; c += CS) {
    double h[DE], kc[NDA];
#pragma unroll
    for (int k = 0; k < DE; ++k) h[k] = hk[k];
#pragma unroll
    for (int k = 0; k < ND; ++k) kc[k] = hk[DE + k];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const dbl2 vv = ld_stream(sp + r0[q]);
      double p0 = vv.x, p1 = vv.y;
#pragma unroll
      for (int k = 0; k < ND; ++k) { p0 = fma(-ks[q][0][k], kc[k], p0); p1 = fma(-ks[q][1][k], kc[k], p1); }
#pragma unroll
      for (int k = 0; k < DE; ++k) { acc[q][0][k] = fma(p0, h[k], acc[q][0][k]); acc[q][1][k] = fma(p1, h[k], acc[q][1][k]); }
      if (WR) { dbl2 o; o.x = p0; o.y = p1; st_stream(dp + r0[q], o); }
    }
    sp += colstep; dp += colstep; hk += hkstep;
  }
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
#pragma unroll
    for (int k = 0; k < DE; ++k) {
      out_acc[(size_t)k * mc + r0[q]] = acc[q][0][k];
      out_acc[(size_t)k * mc + r0[q] + 1] = acc[q][1][k];
    }
  }
}

// The same stream with the pending column factors of the NS sets passing through a double-buffered LDS stage of kKBlock
// columns (KB variants).  All four waves of the workgroup run the block loop together (it has one barrier per block): the
// factors of block b + 1 are fetched into registers before block b streams and parked in the other stage afterwards.
// HK holds [H(D) | X(E)] per column only.  acc_ld: row stride of out_acc (mc for the per-phase partials, ldx when the
// accumulators go straight to PHt).
template <typename TS, int D, int E, int CPL, int UC, int NS, bool WR>
__device__ __forceinline__ void stream_core_blocked(const TS* __restrict__ src, TS* __restrict__ dst,
                                                    const double* __restrict__ HK, double* __restrict__ Kst,
                                                    const SetPtrs<(NS > 0 ? NS : 1)> Fsets, int ldx, int n, int nb, int mc,
                                                    int chunk0, int chunk_stride, int CS, int wc, int lane, int tid,
                                                    double* __restrict__ out_acc, int acc_ld) {
  constexpr int DE = D + E, ND = NS * D, NDA = ND > 0 ? ND : 1;
  constexpr int kPer = (NDA + 3) / 4;                                   // staged values per thread and block
  static_assert(kKBlock == 64, "one lane per column of a block");
  double acc[CPL][2][DE];
  double ks[CPL][2][NDA];
  int r0[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    r0[q] = (chunk0 + q * chunk_stride) * kChunkRows + 2 * lane;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
      for (int k = 0; k < DE; ++k) acc[q][e][k] = 0.0;
#pragma unroll
      for (int sset = 0; sset < NS; ++sset)
#pragma unroll
        for (int k = 0; k < D; ++k) ks[q][e][sset * D + k] = Fsets.p[sset][(size_t)k * ldx + nb + r0[q] + e];
    }
  }
  const size_t colstep = (size_t)CS * mc;
  const int nblk = (n + kKBlock - 1) / kKBlock;
  // stage entry (column cc of the block, factor k) at cc * ND + k.  Lane l fetches column l of the block; factor k is
  // fetched by wave k % 4 (static loop, wave-uniform predicate: no dynamic indexing of the set pointers)
  const int wave_id = tid >> 6;
  auto fetch = [&](int b, double (&v)[kPer]) {
    const int c = min(b * kKBlock + lane, n - 1);
#pragma unroll
    for (int k = 0; k < ND; ++k)
      if ((k & 3) == wave_id) v[k >> 2] = Fsets.p[NS > 0 ? k / D : 0][(size_t)(D + k % D) * ldx + c];
  };
  auto park = [&](int b, const double (&v)[kPer]) {
    double* st = Kst + (size_t)(b & 1) * kKBlock * NDA;
#pragma unroll
    for (int k = 0; k < ND; ++k)
      if ((k & 3) == wave_id) st[(size_t)lane * NDA + k] = v[k >> 2];
  };
  double pre[kPer];
  fetch(0, pre);
  park(0, pre);
  __syncthreads();
  for (int b = 0; b < nblk; ++b) {
    if (b + 1 < nblk) fetch(b + 1, pre);
    const double* st = Kst + (size_t)(b & 1) * kKBlock * NDA;
    const int cb = b * kKBlock, ce = min(n, cb + kKBlock);
    // first column of this wave inside the block: the smallest c >= cb with c % CS == wc
    int c = cb + ((wc - cb % CS) + CS) % CS;
    const TS* sp = src + (size_t)c * mc;
    TS* dp = dst + (size_t)c * mc;
    const double* hk = HK + (size_t)c * DE;
    const int hkstep = CS * DE;
    for (; c + (UC - 1) * CS < ce; c += UC * CS) {
      typename Pair<TS>::type v[UC][CPL];
#pragma unroll
      for (int u = 0; u < UC; ++u)
#pragma unroll
        for (int q = 0; q < CPL; ++q) v[u][q] = ld_stream_raw<TS>(sp + u * colstep + r0[q]);
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        double h[DE], kc[NDA];
#pragma unroll
        for (int k = 0; k < DE; ++k) h[k] = hk[u * hkstep + k];
#pragma unroll
        for (int k = 0; k < ND; ++k) kc[k] = st[(size_t)(c + u * CS - cb) * NDA + k];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
          double p0 = (double)v[u][q].x, p1 = (double)v[u][q].y;
#pragma unroll
          for (int k = 0; k < ND; ++k) { p0 = fma(-ks[q][0][k], kc[k], p0); p1 = fma(-ks[q][1][k], kc[k], p1); }
#pragma unroll
          for (int k = 0; k < DE; ++k) { acc[q][0][k] = fma(p0, h[k], acc[q][0][k]); acc[q][1][k] = fma(p1, h[k], acc[q][1][k]); }
          if (WR) { dbl2 o; o.x = p0; o.y = p1; st_stream(dp + u * colstep + r0[q], o); }
        }
      }
      sp += UC * colstep; dp += UC * colstep; hk += UC * hkstep;
    }
    for (; c < ce; c += CS) {
      double h[DE], kc[NDA];
#pragma unroll
      for (int k = 0; k < DE; ++k) h[k] = hk[k];
#pragma unroll
      for (int k = 0; k < ND; ++k) kc[k] = st[(size_t)(c - cb) * NDA + k];
#pragma unroll
      for (int q = 0; q < CPL; ++q) {
        const dbl2 vv = ld_stream(sp + r0[q]);
        double p0 = vv.x, p1 = vv.y;
#pragma unroll
        for (int k = 0; k < ND; ++k) { p0 = fma(-ks[q][0][k], kc[k], p0); p1 = fma(-ks[q][1][k], kc[k], p1); }
#pragma unroll
        for (int k = 0; k < DE; ++k) { acc[q][0][k] = fma(p0, h[k], acc[q][0][k]); acc[q][1][k] = fma(p1, h[k], acc[q][1][k]); }
        if (WR) { dbl2 o; o.x = p0; o.y = p1; st_stream(dp + r0[q], o); }
      }
      sp += colstep; dp += colstep; hk += hkstep;
    }
    if (b + 1 < nblk) park(b + 1, pre);
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
#pragma unroll
    for (int k = 0; k < DE; ++k) {
      out_acc[(size_t)k * acc_ld + r0[q]] = acc[q][0][k];
      out_acc[(size_t)k * acc_ld + r0[q] + 1] = acc[q][1][k];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// THE step kernel: one workgroup (4 wave64) per particle slot.
//   E = 0 : particleFilter.m:100-204 / particleSmoother.m:124-340 (covariance-form weights)
//   E = 1 : particleSmootherInformationForm.m:274-335 -- additionally streams P*ivec.  The reference also needs P*ivecPlus with
//           ivecPlus = ivec + H' R^-1 y (:292): that is P*ivec + (P H')(R^-1 y), formed from the accumulated columns instead of
//           streamed (r05; as rbpf_step_sym.hip does).  Same algebra, one right-hand side less in the stream -- and the two
//           quadratic forms of the importance weight (:301-303) then SHARE the rounding of P*ivec, which cancels in their difference:
//           against the extended-precision arbiter the weights of dense-radio went from 4.5e-9 (both products streamed; the fp64
//           C restatement: 2.9e-9) to the level of the block-lower kernel
// ---------------------------------------------------------------------------------------------
#ifndef RBPF_MINWAVES
#define RBPF_MINWAVES 1     // min waves per SIMD requested from the register allocator (tuning)
#endif
// UFX: extra unroll of the covariance stream for float storage when a wave owns two row chunks of WHOLE columns
// (RS = 4, CS = 1: n >= 1024); measured at n = 1027: 1: 0.62, 2: 0.39, 3: 0.68, 4: 0.76, 6: 0.67, 8: 0.70 M/s.  With
// CS = 4 (n = 259) the same factor costs a third of the throughput, hence a launch-time choice.
// KB: the pending column factors go through the blocked LDS stage (stream_core_blocked) instead of a record per column.
template <typename TS, int D, int E, int CPL, int NS, bool WR, int UFX = 1, bool KB = false>
__global__ __launch_bounds__(kThreads, RBPF_MINWAVES) void step_kernel(const StepArgs a) {
  extern __shared__ double smem[];
  constexpr int DE = D + E, ND = NS * D, REC = KB ? DE : DE + ND, NSA = NS > 0 ? NS : 1;
  const ModelDev& M = a.mdl;
  const Layout& Ly = a.lay;
  const int n = Ly.n, nb = Ly.nb, mc = Ly.mc, ldx = Ly.ldx, ldb = Ly.ldb;
  const int N = a.N;
  // children are processed in ancestor order so that siblings' reads of the same covariance hit the
  // Infinity Cache; the order only permutes the schedule, slot i still reads / writes slot i's data.
  // propagate_kernel resolved the indirections of this workgroup into one descriptor.
  const int pos = xcd_position((int)blockIdx.x, (int)gridDim.x);   // rbpf_internal.hpp: a family of siblings on ONE XCD
  const int* pre_i = a.pre_i + (size_t)pos * kPreInts;
  if (a.phase >= 0 && pre_i[5] != a.phase) return;     // single-bank flush: not this launch's share (workgroup-uniform)
  const int i = pre_i[0];
  const int dslot = WR ? pre_i[4] : i;                         // bank entry the rewritten matrix goes to
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LdsPlan lp = lds_plan(n, D, E, NS, ldx, Ly.CS, mc, M.ktot, KB ? 1 : 0);
  double* HK = smem + lp.off_HK;        // per column c: H[0..D) | X[0..E) | Kcol of every pending set [NS][D] (not with KB)
  double* xls = smem + lp.off_xl;
  double* PHt = smem + lp.off_PHt;      // [DE][ldx]
  double* parts = smem + lp.off_parts;  // [CS][DE][mc]
  double* tabS = smem + lp.off_tab;
  double* tabC = tabS + (M.ktot > 0 ? M.ktot : 1);
  double* misc = smem + lp.off_misc;    // 0..7 xn_new, 8..16 Rnb, 20.. epilogue broadcast
  double* red = smem + lp.off_red;

#ifdef RBPF_STAMPS
#define RBPF_KSTAMP(k) if (blockIdx.x == 4000 && threadIdx.x == 0 && a.stamps) a.stamps[k] = __builtin_amdgcn_s_memrealtime()
#else
#define RBPF_KSTAMP(k)
#endif
  RBPF_KSTAMP(0);
  const int anc = pre_i[1];      // ancestor id for the non-linear / information-form state banks
  const int ancb = pre_i[2];     // ancestor id in the map bank (local | remote records)
  // sources of the ancestor's map state: the local bank, or a received record
  const bool remote = a.rec != nullptr && ancb >= a.n_bank_local;          // mean / legacy factors in a record
  const double* recp = remote ? a.rec + (size_t)(ancb - a.n_bank_local) * a.rec_stride : nullptr;
  // multi-step lazy update: the stored ("base") matrix of the ancestor's lineage may live in another slot
  const int baseb = pre_i[3];
  const bool remoteP = a.rec != nullptr && baseb >= a.n_bank_local;        // stored matrix in a (persisting) record
  const double* recP = remoteP ? a.rec + (size_t)(baseb - a.n_bank_local) * a.rec_stride : nullptr;
  // (a record keeps the covariance blocks in the stored type; rec_off_B is in doubles)
  const TS* srcT = remoteP ? reinterpret_cast<const TS*>(recP) : reinterpret_cast<const TS*>(a.Pt_old) + (size_t)baseb * a.Pt_old_stride;
  const TS* srcB = remoteP ? reinterpret_cast<const TS*>(recP + a.rec_off_B) : reinterpret_cast<const TS*>(a.Pb_old) + (size_t)baseb * a.Pb_old_stride;
  const double* srcX = remote ? recp + a.rec_off_X : a.xl_old + (size_t)ancb * a.xl_old_stride;
  // pending factor sets (KS rows then K columns, [2][D][ldx] each), oldest first
  SetPtrs<NSA> srcFs;
#pragma unroll
  for (int sset = 0; sset < NSA; ++sset) srcFs.p[sset] = nullptr;
#pragma unroll
  for (int sset = 0; sset < NS; ++sset) {
    if (a.fset[sset]) srcFs.p[sset] = a.fset[sset] + (size_t)pre_i[kPreSet0 + sset] * 2 * D * ldx;
    else srcFs.p[sset] = remote ? recp + a.rec_off_F : a.F_old + (size_t)ancb * 2 * D * ldx;
  }
  const int nN = M.nN;

  // ---- A: fetch the propagated non-linear state (propagate_kernel ran first), stage xl / pending K / ivec ----
  if (tid < kPreDoubles) misc[tid] = a.pre_d[(size_t)pos * kPreDoubles + tid];   // xn_new[0..8), Rnb[8..17)
  {
    // all loads of a pass are issued before the first LDS store (clamped indices, predicated stores): the
    // sources are scattered small arrays, so this phase is pure latency
    const double* xl_src = srcX;
    const double* iv = (E > 0) ? (remote ? recp + a.rec_off_I : a.ivec_old + (size_t)ancb * a.ivec_old_stride) : nullptr;
    constexpr int PB = 2;                                   // columns per thread per pass
    for (int c0 = tid; c0 < n; c0 += PB * kThreads) {
      double xv[PB], ivv[PB], kv[PB][ND > 0 ? ND : 1];
#pragma unroll
      for (int u = 0; u < PB; ++u) {
        const int c = min(c0 + u * kThreads, n - 1);
        xv[u] = xl_src[c];
        ivv[u] = (E > 0) ? iv[c] : 0.0;
        if (!KB) {
#pragma unroll
          for (int sset = 0; sset < NS; ++sset)
#pragma unroll
            for (int k = 0; k < D; ++k) kv[u][sset * D + k] = srcFs.p[sset][(size_t)(D + k) * ldx + c];
        }
      }
#pragma unroll
      for (int u = 0; u < PB; ++u) {
        const int c = c0 + u * kThreads;
        if (c < n) {
          xls[c] = xv[u];
          if (!KB) {
#pragma unroll
            for (int k = 0; k < ND; ++k) HK[c * REC + DE + k] = kv[u][k];
          }
          if (E > 0) HK[c * REC + D] = ivv[u];
        }
      }
    }
  }
  __syncthreads();

  RBPF_KSTAMP(1);
  // ---- B: per-axis sin/cos tables of the reduced-rank basis at the new position ----
  for (int q = tid; q < M.ktot; q += kThreads) basis_table_entry(M, q, misc, tabS, tabC);
  __syncthreads();

  RBPF_KSTAMP(2);
  // ---- C: measurement Jacobian H_i, column per thread (+ ivecPlus = ivec + dyi'/R*yt', :292) ----
  double Riy[D];                                               // R^-1 y
  if (E > 0) {
#pragma unroll
    for (int aa = 0; aa < D; ++aa) {
      double s = 0.0;
#pragma unroll
      for (int bb = 0; bb < D; ++bb) s = fma(model_Rinv<D>(M, aa + D * bb), a.y[bb], s);
      Riy[aa] = s;
    }
  }
  {
    for (int c = tid; c < n; c += kThreads) {
      double h[D];
      if (D > 3 || a.H_ext != nullptr) {                       // (no built-in family is wider than 3: launch_step refuses)
#pragma unroll
        for (int k = 0; k < D; ++k) h[k] = a.H_ext[((size_t)i * D + k) * ldx + c];         // measModel was evaluated on the host
      } else {
        H_column<D>(M, c, tabS, tabC, &misc[8], h);
      }
#pragma unroll
      for (int k = 0; k < D; ++k) HK[c * REC + k] = h[k];
      if (E > 0) {
        double s = HK[c * REC + D];                                          // ivecPlus (:292), the new information vector (:333)
#pragma unroll
        for (int k = 0; k < D; ++k) s = fma(h[k], Riy[k], s);
#pragma unroll
        for (int k = 0; k < D; ++k) a.Hb_new[((size_t)i * D + k) * ldx + c] = h[k];
        a.ivec_new[(size_t)i * ldx + c] = s;
      }
    }
  }
  __syncthreads();

  RBPF_KSTAMP(3);
  // ---- D: stream the covariance once: apply pending downdate, store, accumulate P+ [H' X] ----
  {
    const int wr = wave % Ly.RS, wc = wave / Ly.RS;
#ifndef RBPF_UF32
#define RBPF_UF32 2
#endif
    // a float load brings half the bytes: twice the columns in flight keep the same bytes outstanding
    constexpr int kUF = ((sizeof(TS) == 4 && CPL <= 1) ? RBPF_UF32 : 1) * UFX;
    if (KB) {
      // every wave of the workgroup runs the block loop (launch-time guarantee: RS * CS == 4 waves, no remainder chunk)
      const TS* src = srcT;
      TS* dst = reinterpret_cast<TS*>(a.Pt_new) + (size_t)dslot * Ly.szT;
      const bool direct = Ly.CS == 1;                       // one column phase: accumulators go straight to PHt
      double* out_acc = direct ? PHt + nb : parts + (size_t)wc * DE * mc;
      stream_core_blocked<TS, D, E, (CPL > 0 ? CPL : 1), kUF * step_uc(D, CPL), NS, WR>(
          src, dst, HK, smem + lp.off_kst, srcFs, ldx, n, nb, mc, wr, Ly.RS, Ly.CS, wc, lane, tid, out_acc, direct ? ldx : mc);
    } else if (mc > 0 && wc < Ly.CS) {
      const TS* src = srcT;
      TS* dst = reinterpret_cast<TS*>(a.Pt_new) + (size_t)dslot * Ly.szT;
      double* out_acc = parts + (size_t)wc * DE * mc;
      // CPL full rounds of RS chunks (every wave), then one remainder chunk for the first CH % RS waves:
      // both decisions are wave-uniform, so the streaming loops are branch-free
      if (CPL > 0)
        stream_core<TS, D, E, (CPL > 0 ? CPL : 1), kUF * step_uc(D, CPL), NS, WR>(src, dst, HK, srcFs, ldx, n, nb, mc, wr, Ly.RS, Ly.CS, wc, lane, out_acc);
      const int rem = Ly.CH - CPL * Ly.RS;
      if (wr < rem)
        stream_core<TS, D, E, 1, kUF * step_uc(D, 1), NS, WR>(src, dst, HK, srcFs, ldx, n, nb, mc, CPL * Ly.RS + wr, 1, Ly.CS, wc, lane, out_acc);
    }
    // border rows (row-major block B): lanes walk columns, wave-reduce per row
    for (int b = wave; b < nb; b += kWaves) {
      const TS* src = srcB + (size_t)b * ldb;
      TS* dst = reinterpret_cast<TS*>(a.Pb_new) + (size_t)dslot * Ly.szB + (size_t)b * ldb;
      double ksb[ND > 0 ? ND : 1];
#pragma unroll
      for (int sset = 0; sset < NS; ++sset)
#pragma unroll
        for (int k = 0; k < D; ++k) ksb[sset * D + k] = srcFs.p[sset][(size_t)k * ldx + b];
      double accb[DE];
#pragma unroll
      for (int k = 0; k < DE; ++k) accb[k] = 0.0;
      for (int c = 2 * lane; c < ldb; c += 128) {
        const dbl2 vv = ld_pair<TS>(src + c);
        double p[2] = {vv.x, vv.y};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int cc = c + e;
          if (cc < n) {
#pragma unroll
            for (int k = 0; k < ND; ++k) {
              // pending column factor K(cc, k): from the per-column record, or (KB) straight from the factor set
              const double kcv = KB ? srcFs.p[NS > 0 ? k / D : 0][(size_t)(D + k % D) * ldx + cc] : HK[cc * REC + DE + k];
              p[e] = fma(-ksb[k], kcv, p[e]);
            }
#pragma unroll
            for (int k = 0; k < DE; ++k) accb[k] = fma(p[e], HK[cc * REC + k], accb[k]);
          }
        }
        if (WR) { dbl2 o; o.x = p[0]; o.y = p[1]; st_pair<TS>(dst + c, o); }
      }
#pragma unroll
      for (int k = 0; k < DE; ++k) {
        const double s = wave_sum(accb[k]);
        if (lane == 0) PHt[(size_t)k * ldx + b] = s;
      }
    }
  }
  __syncthreads();
  if (mc > 0 && !(KB && Ly.CS == 1)) {
    // fixed-order combine of the column phases (deterministic)
    for (int r = tid; r < mc; r += kThreads) {
#pragma unroll
      for (int k = 0; k < DE; ++k) {
        double s = parts[(size_t)k * mc + r];
        for (int w = 1; w < Ly.CS; ++w) s += parts[((size_t)w * DE + k) * mc + r];
        PHt[(size_t)k * ldx + nb + r] = s;
      }
    }
    __syncthreads();
  }

  RBPF_KSTAMP(4);
  // ---- E: innovation covariance S = H (P H') + R, innovation e = y - H xl (+ quadratic forms) ----
  constexpr int NRED = D * D + D + 2 * E, RST = red_stride(D, E), MQ = misc_q(D);
  {
    double part[NRED];
#pragma unroll
    for (int q = 0; q < NRED; ++q) part[q] = 0.0;
    for (int r = tid; r < n; r += kThreads) {
      double h[D], ph[D];
#pragma unroll
      for (int k = 0; k < D; ++k) { h[k] = HK[r * REC + k]; ph[k] = PHt[(size_t)k * ldx + r]; }
      const double x = xls[r];
#pragma unroll
      for (int bb = 0; bb < D; ++bb)
#pragma unroll
        for (int aa = 0; aa < D; ++aa) part[aa + D * bb] = fma(h[aa], ph[bb], part[aa + D * bb]);
#pragma unroll
      for (int aa = 0; aa < D; ++aa) part[D * D + aa] = fma(h[aa], x, part[D * D + aa]);
      if (E > 0) {
        // ivec'*P*ivec and ivecPlus'*P*ivecPlus (:301-303) with P = the (downdated) prior covariance; P*ivecPlus = P*ivec + (P H')(R^-1 y)
        const double iv = HK[r * REC + D], piv = PHt[(size_t)D * ldx + r];
        double ivp = iv, pivp = piv;
#pragma unroll
        for (int k = 0; k < D; ++k) { ivp = fma(h[k], Riy[k], ivp); pivp = fma(ph[k], Riy[k], pivp); }
        part[D * D + D] = fma(iv, piv, part[D * D + D]);
        part[D * D + D + 1] = fma(ivp, pivp, part[D * D + D + 1]);
      }
    }
#pragma unroll
    for (int q = 0; q < NRED; ++q) {
      const double s = wave_sum(part[q]);
      if (lane == 0) red[wave * RST + q] = s;
    }
  }
  __syncthreads();
  if (tid == 0) {
    // d <= 3: S, chol(S), the innovation and the solve live in registers and are copied to their broadcast slots below.  Wider: thread
    // 0 works in those slots of misc directly (private arrays of d*d doubles walked by loops would sit in scratch memory).
    constexpr int DR = D <= 3 ? D : 1;
    double SSr[DR * DR], er[DR], cSr[DR * DR], vr[DR];
    double *SS = SSr, *e = er, *cS = cSr, *v = vr;
    if constexpr (D > 3) { SS = misc + misc_SS(D); e = misc + misc_e(D); cS = misc + misc_cS(D); v = misc + misc_e(D) + D; }
    for (int q = 0; q < D * D; ++q) {
      double s = red[q];
      for (int w = 1; w < kWaves; ++w) s += red[w * RST + q];
      SS[q] = s + model_R<D>(M, q);                                         // particleFilter.m:141
    }
    for (int q = 0; q < D; ++q) {
      double s = red[D * D + q];
      for (int w = 1; w < kWaves; ++w) s += red[w * RST + D * D + q];
      e[q] = a.y[q] - s;                                                    // :140
    }
    bool ok = chol_lower_small<D>(SS, cS);                                  // :145
    if (!ok) {
      if constexpr (D <= 3) {
        double SJ[D * D];
        for (int q = 0; q < D * D; ++q) SJ[q] = SS[q];
        for (int q = 0; q < D; ++q) SJ[q + D * q] += M.jitter;              // :147
        ok = chol_lower_small<D>(SJ, cS);
      } else {                                                              // the same on S itself; its diagonal is put back (K*SS uses S)
        for (int q = 0; q < D; ++q) { v[q] = SS[q + D * q]; SS[q + D * q] += M.jitter; }
        ok = chol_lower_small<D>(SS, cS);
        for (int q = 0; q < D; ++q) SS[q + D * q] = v[q];
      }
    }
    double lw = 0.0, sl = 0.0;
    if (ok) {
      fwd_subst<D>(cS, e, v);                                               // :149
      double vv = 0.0;
      for (int q = 0; q < D; ++q) { sl += log(cS[q + D * q]); vv += v[q] * v[q]; }
      lw = -sl - 0.5 * vv + M.logconst;                                     // :150
    } else {
      atomicOr(a.status, 1);
      lw = nan("");
      for (int q = 0; q < D * D; ++q) cS[q] = 0.0;
      for (int q = 0; q < D; ++q) cS[q + D * q] = 1.0;
    }
    if (E == 0) a.logw[i] = lw;
    if constexpr (D <= 3) {
      for (int q = 0; q < D * D; ++q) { misc[misc_cS(D) + q] = cS[q]; misc[misc_SS(D) + q] = SS[q]; }
      for (int q = 0; q < D; ++q) misc[misc_e(D) + q] = e[q];
    }
    if (E > 0) {
      double qa = red[D * D + D], qb = red[D * D + D + 1];
      for (int w = 1; w < kWaves; ++w) { qa += red[w * RST + D * D + D]; qb += red[w * RST + D * D + D + 1]; }
      misc[MQ] = qa; misc[MQ + 1] = qb; misc[MQ + 2] = ok ? sl : nan("");
    }
  }
  __syncthreads();

  RBPF_KSTAMP(5);
  // ---- F: Kalman gain rows, mean update, new pending factors (particleFilter.m:194-198) ----
  {
    // (d <= 3: copies in registers; wider: read where thread 0 left them -- every lane the same address, an LDS broadcast)
    constexpr int DR = D <= 3 ? D : 1;
    double cSr[DR * DR], SSr[DR * DR], er[DR];
    const double *cS = misc + misc_cS(D), *SS = misc + misc_SS(D), *e = misc + misc_e(D);
    if constexpr (D <= 3) {
#pragma unroll
      for (int q = 0; q < D * D; ++q) { cSr[q] = misc[misc_cS(D) + q]; SSr[q] = misc[misc_SS(D) + q]; }
#pragma unroll
      for (int q = 0; q < D; ++q) er[q] = misc[misc_e(D) + q];
      cS = cSr; SS = SSr; e = er;
    }
    double* KSn = a.F_new + ((size_t)i * 2 + 0) * D * ldx;
    double* Kn = a.F_new + ((size_t)i * 2 + 1) * D * ldx;
    if (tid == 0) {
      // lineage bookkeeping of the multi-step lazy update: where this particle's stored matrix and its
      // surviving pending sets live (a flush makes them all obsolete)
      if (a.base_new) a.base_new[i] = WR ? dslot : (a.share_flush ? pre_i[4] : baseb);
      if (!WR) {
#pragma unroll
        for (int sset = 0; sset < NS; ++sset)
          if (a.fset_idx_new[sset]) a.fset_idx_new[sset][i] = pre_i[kPreSet0 + sset];
      }
      if (a.fself_idx_new) a.fself_idx_new[i] = i;
    }
    double* xln = a.xl_new + (size_t)i * ldx;
    double uK[D];
#pragma unroll
    for (int k = 0; k < D; ++k) uK[k] = 0.0;
    for (int r = tid; r < n; r += kThreads) {
      double ph[D], u[D], kk[D];
#pragma unroll
      for (int k = 0; k < D; ++k) ph[k] = PHt[(size_t)k * ldx + r];
      fwd_subst<D>(cS, ph, u);          // (P H') / cS'
      bwd_subst_T<D>(cS, u, kk);        // ... / cS   -> row r of K
      double xn_ = xls[r];
#pragma unroll
      for (int k = 0; k < D; ++k) xn_ = fma(kk[k], e[k], xn_);              // :197
      xln[r] = xn_;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s = fma(kk[k], SS[k + D * j], s);       // row r of K*SS
        KSn[(size_t)j * ldx + r] = s;
        Kn[(size_t)j * ldx + r] = kk[j];
      }
      if (E > 0) {
        double ip = HK[r * REC + D];
#pragma unroll
        for (int k = 0; k < D; ++k) ip = fma(HK[r * REC + k], Riy[k], ip);
#pragma unroll
        for (int k = 0; k < D; ++k) uK[k] = fma(ip, kk[k], uK[k]);          // ivecPlus' * K
      }
    }
    if (E > 0) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double s = wave_sum(uK[k]);
        if (lane == 0) red[wave * RST + k] = s;
      }
      __syncthreads();
      if (tid == 0) {
        double ur[DR];
        double* u = ur;
        if constexpr (D > 3) u = misc + misc_e(D) + D;                      // the spare d doubles
        for (int k = 0; k < D; ++k) { double s = red[k]; for (int w = 1; w < kWaves; ++w) s += red[w * RST + k]; u[k] = s; }
        double corr = 0.0;                                                  // ivecPlus' * (K*SS*K') * ivecPlus
        for (int bb = 0; bb < D; ++bb) {
          double t = 0.0;
          for (int aa = 0; aa < D; ++aa) t = fma(u[aa], SS[aa + D * bb], t);
          corr = fma(t, u[bb], corr);
        }
        const double qa = misc[MQ], qbp = misc[MQ + 1] - corr, sl = misc[MQ + 2];
        const double hld = remote ? recp[a.rec_off_hld] : a.hld_old[(size_t)ancb * a.hld_old_stride];
        const double hldp = -sl + M.halfLogDetR + hld;                       // :298
        double yRy = 0.0;
        for (int bb = 0; bb < D; ++bb) {
          double t = 0.0;
          for (int aa = 0; aa < D; ++aa) t = fma(a.y[aa], model_Rinv<D>(M, aa + D * bb), t);
          yRy = fma(t, a.y[bb], yRy);
        }
        // :301-304   (1/2*log((2*pi)^ny*det(R)) = -logconst + halfLogDetR)
        a.logw[i] = -0.5 * qa - hld + hldp + 0.5 * qbp - 0.5 * yRy - (-M.logconst + M.halfLogDetR);
        a.hld_new[i] = hldp;
        a.qf_new[i] = qbp;
      }
    }
  }
  __syncthreads();
  RBPF_KSTAMP(6);
}

template <typename TS, int D, int E, int CPL, int NS, bool WR, int UFX, bool KB>
static hipError_t launch_step_k(const StepArgs& a, size_t lds, hipStream_t s) {
  static std::atomic<uint64_t> attr_done{0};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&step_kernel<TS, D, E, CPL, NS, WR, UFX, KB>), 160 * 1024, attr_done)) return e;
  hipLaunchKernelGGL((step_kernel<TS, D, E, CPL, NS, WR, UFX, KB>), dim3(a.N), dim3(kThreads), lds, s, a);
  return hipGetLastError();
}

template <typename TS, int D, int E, int CPL, int NS, bool WR>
static hipError_t launch_step_t(const StepArgs& a, hipStream_t s) {
  const size_t lds = step_lds_bytes(a.mdl, a.lay, E, NS);
  // launch-time unroll choices that depend on the wave decomposition (see step_kernel): float storage with whole
  // columns per wave and two row chunks (n >= 1024) x4; double storage in the 2 x 2 decomposition (the flush kernel of
  // the lazy update at n = 259) x2 (8.2 vs 7.7 M particle-steps/s at N = 8192)
  // (both belong to fp32 storage and to the lazy update, which only the widths 1 and 3 have)
  constexpr int kWide = (D != 1 && D != 3) ? 1 : (sizeof(TS) == 4 && CPL == 2) ? 4 : ((sizeof(TS) == 8 && CPL == 1 && E == 0) ? 2 : 1);
  bool wide = false;
  if constexpr (kWide > 1) wide = (sizeof(TS) == 4) ? (a.lay.CS == 1) : (a.lay.CS == 2 && a.lay.RS == 2);
  // pending factors through the blocked LDS stage when the per-column records would leave one workgroup per CU
  if constexpr (NS >= 1 && CPL >= 1 && CPL <= 2) {
    if (step_use_blocked(a.mdl, a.lay, E, NS)) {
      if constexpr (kWide > 1) { if (wide) return launch_step_k<TS, D, E, CPL, NS, WR, kWide, true>(a, lds, s); }
      return launch_step_k<TS, D, E, CPL, NS, WR, 1, true>(a, lds, s);
    }
  }
  if constexpr (kWide > 1) { if (wide) return launch_step_k<TS, D, E, CPL, NS, WR, kWide, false>(a, lds, s); }
  return launch_step_k<TS, D, E, CPL, NS, WR, 1, false>(a, lds, s);
}

template <typename TS, int D, int E, int NS, bool WR>
static hipError_t launch_step_cpl(const StepArgs& a, hipStream_t s) {
  switch (a.lay.CPL) {
    case 0: return launch_step_t<TS, D, E, 0, NS, WR>(a, s);
    case 1: return launch_step_t<TS, D, E, 1, NS, WR>(a, s);
    case 2: return launch_step_t<TS, D, E, 2, NS, WR>(a, s);
    case 3: return launch_step_t<TS, D, E, 3, NS, WR>(a, s);
    default: return hipErrorInvalidValue;
  }
}

// The generic family's widths other than 1 and 3 (rbpf_step_wide_*.hip, one unit per pair of widths so that they compile side by
// side): fp64 full squares, one pending set rewritten every step -- filter (E = 0) and information form (E = 1).
template <int D>
static hipError_t launch_step_wide_t(const StepArgs& a, hipStream_t s) {
  static_assert(D >= 1 && D <= 8, "misc / red slots and the one-thread Cholesky are laid out for n_y <= 8");
  if (a.fp32 || a.lay.sym || !a.write_base || a.n_sets > 1 || a.H_ext == nullptr || (D > 3 && a.mdl.Rdev == nullptr)) return hipErrorInvalidValue;
  if (a.info) return a.n_sets ? launch_step_cpl<double, D, 1, 1, true>(a, s) : launch_step_cpl<double, D, 1, 0, true>(a, s);
  return a.n_sets ? launch_step_cpl<double, D, 0, 1, true>(a, s) : launch_step_cpl<double, D, 0, 0, true>(a, s);
}

}  // namespace rbpf
