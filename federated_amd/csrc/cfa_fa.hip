// cfa_fa.hip — one server-federation epoch of a device-resident TF1 population under the CFA-FA
// driver (cfa_fa_population_round_f32): the server's fp64 fold of the D published models and every
// device's pull toward the folded model, in one launch.
#include <type_traits>

#include "cfa_internal.h"
#include "cfa_fa_shape.h"

// The chain is numpy's: every fp64 product and sum rounded on its own (the Makefile compiles every
// .hip file with -ffp-contract=off; repeated here because every bit-for-bit claim below rests on it).
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------
// Server epoch (federated_sample_CNN_CFA_FA.py): the server folds the models the D devices
// published, in device order, into its fp64 model s (:86-89 at epoch 0, s <- s + b_d * x_d;
// :103-110 / :130-133 later, s <- s + (eps * b_d) * (x_d - s)), then every device takes
// W <- W + eps2 * (s - W) with the folded s (:280-283), rounded once to the fp32 it is fed back as;
// at epoch 0 the devices keep their models. The column-ownership scheme of cfa_fedavg.hip: a lane
// owns its columns for the whole launch, loads s, streams the D input rows and folds them in row
// order (the chain is sequential in s, the row loads are not: B rows' loads of U elements each are
// issued ahead of their folds), stores s, then writes the D output rows. No other lane reads or
// writes those columns, so there are no atomics and no workspace.
//
// What is read twice: with D <= B the rows stay in registers between the fold and the client step
// and every input element is loaded once. With D > B the client step loads all D input rows a
// second time (the fold's loads are then ordinary ones, so that the second read of a workgroup's
// few KiB per row can come from the caches; the second read itself is nontemporal). s and coef
// are read once either way.
//
// Rows and s whose bases and pitches are 16-byte aligned go as float4 / two double2 per lane
// element; anything else takes the same operations one float / double at a time.
// ------------------------------------------------------------------------------------------
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

struct FaArgs {
  const float* in;     // [D, in_pitch]
  float* out;          // [D, out_pitch]
  double* s;           // [P]
  const double* coef;  // [D]: b_d (init) or eps * b_d
  long long in_pitch, out_pitch;
  double eps2;
  int D, mode;
};

// The fp64 form of a lane's column element.
template <typename T>
struct Wide {
  using type = double;
};
template <>
struct Wide<f4> {
  using type = d4;
};

template <typename T>
__device__ __forceinline__ typename Wide<T>::type widen(T x) {
  if constexpr (std::is_same_v<T, f4>) return __builtin_convertvector(x, d4);
  else return (double)x;
}
template <typename T>
__device__ __forceinline__ T narrow(typename Wide<T>::type w) {  // one rounding to nearest even
  if constexpr (std::is_same_v<T, f4>) return __builtin_convertvector(w, f4);
  else return (float)w;
}

template <typename T, bool NT>
__device__ __forceinline__ T ld_x(const float* row, long long i) {
  if constexpr (std::is_same_v<T, f4>) return ld4<NT>(row, i);
  else return row[i];
}
template <typename T, bool NT>
__device__ __forceinline__ void st_x(float* row, long long i, T v) {
  if constexpr (std::is_same_v<T, f4>) st4<NT>(row, i, v);
  else row[i] = v;
}
template <typename T>
__device__ __forceinline__ typename Wide<T>::type ld_s(const double* s, long long i) {
  if constexpr (std::is_same_v<T, f4>) {
    const d2* q = reinterpret_cast<const d2*>(s) + 2 * i;
    const d2 lo = q[0], hi = q[1];
    return d4{lo.x, lo.y, hi.x, hi.y};
  } else {
    return s[i];
  }
}
template <typename T>
__device__ __forceinline__ void st_s(double* s, long long i, typename Wide<T>::type v) {
  if constexpr (std::is_same_v<T, f4>) {
    d2* q = reinterpret_cast<d2*>(s) + 2 * i;
    q[0] = d2{v.x, v.y};
    q[1] = d2{v.z, v.w};
  } else {
    s[i] = v;
  }
}

// B rows from row d0 on, the lane's U elements of each at i0 + u * kBlock. d0 is wave-uniform.
template <typename T, int U, int B, bool NT>
__device__ __forceinline__ void fa_load(T (&x)[B][U], const FaArgs& a, int d0, long long i0) {
  const float* const row0 = a.in + (long long)d0 * a.in_pitch;
#pragma unroll
  for (int b = 0; b < B; ++b)
    if (d0 + b < a.D) {
#pragma unroll
      for (int u = 0; u < U; ++u) x[b][u] = ld_x<T, NT>(row0 + b * a.in_pitch, i0 + (long long)u * kBlock);
    }
}

// The whole epoch on the lane's U column elements at i0 + u * kBlock. KEEP: D <= B, the rows of
// the one batch stay in registers for the client step.
template <typename T, int U, int B, bool NT, bool KEEP>
__device__ __forceinline__ void fa_columns(const FaArgs& a, long long i0) {
  using W = typename Wide<T>::type;
  const bool init = a.mode == CFA_FA_INIT;
  W s[U];
#pragma unroll
  for (int u = 0; u < U; ++u) s[u] = ld_s<T>(a.s, i0 + (long long)u * kBlock);
  T x[B][U];
  for (int d0 = 0; d0 < a.D; d0 += B) {
    fa_load<T, U, B, KEEP>(x, a, d0, i0);
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (d0 + b < a.D) {
        const double c = a.coef[d0 + b];  // uniform: a scalar load
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const W xd = widen<T>(x[b][u]);
          if (init) {
            const W t = c * xd;  // numpy: b_d * x_d
            s[u] = s[u] + t;     //        s + (...)
          } else {
            W t = xd - s[u];  // numpy: (x_d - s)
            t = c * t;        //        (eps * b_d) * (...)
            s[u] = s[u] + t;  //        s + (...)
          }
        }
      }
  }
  if (a.D > 0) {
#pragma unroll
    for (int u = 0; u < U; ++u) st_s<T>(a.s, i0 + (long long)u * kBlock, s[u]);
  }
  for (int d0 = 0; d0 < a.D; d0 += B) {
    if constexpr (!KEEP) fa_load<T, U, B, true>(x, a, d0, i0);
    float* const row0 = a.out + (long long)d0 * a.out_pitch;
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (d0 + b < a.D) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          T y = x[b][u];  // epoch 0: the device keeps its model
          if (!init) {
            const W w = widen<T>(y);
            W t = s[u] - w;  // numpy: (s - W)
            t = a.eps2 * t;  //        eps2 * (...)
            y = narrow<T>(w + t);
          }
          st_x<T, NT>(row0 + b * a.out_pitch, i0 + (long long)u * kBlock, y);
        }
      }
  }
}

template <typename T, int U, int B, bool NT>
__device__ __forceinline__ void fa_columns_any(const FaArgs& a, long long i0) {
  if (a.D <= B) fa_columns<T, U, B, NT, true>(a, i0);
  else fa_columns<T, U, B, NT, false>(a, i0);
}

// n column elements of type T (float4: n = P / 4, and block 0 takes the P mod 4 tail as floats).
template <typename T, int U, int B, bool NT>
__global__ __launch_bounds__(kBlock) void fa_round_kernel(FaArgs a, long long n, long long P) {
  const TileWalk<U> tw(n);
  for (const long long base : tw.full_tiles()) fa_columns_any<T, U, B, NT>(a, base);
  if (tw.owns_partial())
    for (const long long i : tw.partial_tile()) fa_columns_any<T, 1, B, NT>(a, i);
  if constexpr (std::is_same_v<T, f4>) {
    if (blockIdx.x == 0 && n * 4 + threadIdx.x < P) fa_columns_any<float, 1, B, false>(a, n * 4 + threadIdx.x);
  }
}

// Launch shape: FaTune of cfa_fa_shape.h. The environment overrides are read at each launch (no
// HIP call: capture-safe), so one process can compare shapes on the same buffers and the tests can
// reach both batch depths and the grid-stride loop; results are identical for every shape.
// CFA_FA_MAX_GRID > 0 caps the workgroups of a launch.
static_assert(kFaBlock == kBlock, "cfa_fa_shape.h counts tiles of kBlock lanes");
static FaTune fa_tune() {
  const FaTune d = kFaDefault;
  FaTune t{env_int("CFA_FA_U", d.u), env_int("CFA_FA_U", d.u_long), env_int("CFA_FA_BATCH", d.batch),
           env_int("CFA_FA_WG_PER_CU", d.wg_per_cu)};
  if (t.u != 1 && t.u != 2 && t.u != 4) t.u = d.u, t.u_long = d.u_long;
  if (t.batch != 4 && t.batch != 8) t.batch = d.batch;
  if (t.wg_per_cu <= 0) t.wg_per_cu = d.wg_per_cu;
  return t;
}
static bool fa_vector_rows(const float* in, size_t in_pitch, const float* out, size_t out_pitch, const double* s) {
  return !((addr(in) | addr(out) | addr(s)) & 15) && in_pitch % 4 == 0 && out_pitch % 4 == 0;
}

template <typename T, int U, int B>
void launch_fa_ub(const FaArgs& a, unsigned grid, bool nt, long long n, long long P, hipStream_t st) {
  if constexpr (std::is_same_v<T, f4>) {
    if (nt) {
      fa_round_kernel<T, U, B, true><<<grid, kBlock, 0, st>>>(a, n, P);
      return;
    }
  }
  fa_round_kernel<T, U, B, false><<<grid, kBlock, 0, st>>>(a, n, P);
}
template <typename T, int U>
void launch_fa_u(const FaArgs& a, const FaTune& t, long long P, hipStream_t st) {
  const long long n = std::is_same_v<T, f4> ? P / 4 : P;
  const long long tile = (long long)kBlock * U;
  cfa_launch_t lc = tune();
  lc.blocks_per_cu = t.wg_per_cu;
  unsigned grid = grid_for((n + tile - 1) / tile, lc);
  const int cap = env_int("CFA_FA_MAX_GRID", 0);
  if (cap > 0 && grid > (unsigned)cap) grid = (unsigned)cap;
  if (t.batch == 8) launch_fa_ub<T, U, 8>(a, grid, fa_nt_store(P), n, P, st);
  else launch_fa_ub<T, U, 4>(a, grid, fa_nt_store(P), n, P, st);
}
template <typename T>
void launch_fa(const FaArgs& a, const FaTune& t, long long P, hipStream_t st) {
  switch (fa_u(P, t)) {
    case 4: launch_fa_u<T, 4>(a, t, P, st); break;
    case 2: launch_fa_u<T, 2>(a, t, P, st); break;
    default: launch_fa_u<T, 1>(a, t, P, st); break;
  }
}

}  // namespace

extern "C" size_t cfa_fa_round_tile(size_t P, int aligned) {
  return (size_t)kBlock * (size_t)fa_u((long long)P, fa_tune()) * (aligned ? 4 : 1);
}

extern "C" int cfa_fa_population_round_f32(float* out, size_t out_pitch, const float* in, size_t in_pitch,
                                           double* s, const double* coef, double eps2, int mode, int D,
                                           size_t P, void* stream) {
  if (D < 0) return fail(CFA_E_INVALID, "negative device count");
  if (mode != CFA_FA_INIT && mode != CFA_FA_ROUND) return fail(CFA_E_INVALID, "unknown CFA-FA mode %d", mode);
  if (in_pitch < P || out_pitch < P)
    return fail(CFA_E_INVALID, "pitch %zu / %zu below P %zu", in_pitch, out_pitch, P);
  if (P == 0) return CFA_OK;
  if (!s || (D > 0 && (!in || !out || !coef))) return fail(CFA_E_INVALID, "null rows, server model or coefficients");
  if (D > 0) {
    const uintptr_t in_end = addr(in) + ((size_t)(D - 1) * in_pitch + P) * sizeof(float);
    const uintptr_t out_end = addr(out) + ((size_t)(D - 1) * out_pitch + P) * sizeof(float);
    if (addr(in) < out_end && addr(out) < in_end) return fail(CFA_E_INVALID, "out overlaps in");
  }
  const FaArgs a{in, out, s, coef, (long long)in_pitch, (long long)out_pitch, eps2, D, mode};
  const FaTune t = fa_tune();
  hipStream_t st = (hipStream_t)stream;
  if (fa_vector_rows(in, in_pitch, out, out_pitch, s)) launch_fa<f4>(a, t, (long long)P, st);
  else launch_fa<float>(a, t, (long long)P, st);
  return check_launch("cfa_fa_round");
}
